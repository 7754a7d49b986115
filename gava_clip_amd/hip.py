"""ctypes binding of libgava_hip.so (include/gava_hip.h).

The product path has NO fallback: if the library is missing or a call is rejected this module
raises.  torch is used only to own device memory and to name the current HIP stream.
"""
import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GAVA_HIP_LIB") or os.path.join(_HERE, "libgava_hip.so")   # env: A/B experiment builds only

PREC_F16, PREC_BF16 = 0, 1
KERNEL_AUTO, KERNEL_256, KERNEL_PAIR, KERNEL_PP = 0, 3, 4, 5     # gava_gemm_args.kernel
EPI_H16, EPI_H16_QGELU, EPI_F32, EPI_F32_PATCH, EPI_H16_QGELU_BWD = 0, 1, 2, 3, 4
UNPATCH_GRAD, UNPATCH_ABSMAX, UNPATCH_L2, UNPATCH_GRAD_X_INPUT = 0, 1, 2, 3      # gava_unpatchify_args.mode
MAX_GRID_FRAMES = 65535      # clips x frames one gava_preprocess_clips / gava_patchify launch covers (its grid's z extent)
PREC_NAMES = {"fp16": PREC_F16, "f16": PREC_F16, "bf16": PREC_BF16}
PREC_TORCH = {PREC_F16: torch.float16, PREC_BF16: torch.bfloat16}

EXPORTS = ["gava_abi_version", "gava_gemm", "gava_layernorm", "gava_attention",
           "gava_vision_workspace_bytes", "gava_vision_forward", "gava_text_workspace_bytes",
           "gava_text_forward", "gava_similarity_head", "gava_convert_h16", "gava_debug_set_buffer",
           "gava_preprocess_clip", "gava_layernorm_backward", "gava_qgelu_backward", "gava_attention_backward",
           "gava_text_forward_train", "gava_vision_forward_train", "gava_attention_backward_workspace_bytes", "gava_vision_forward_keep", "gava_row_stats",
           "gava_probe_fc1_enable", "gava_probe_fc1_read", "gava_clip_geometry", "gava_patchify", "gava_attention_f32",
           "gava_gemm_aligned_walk", "gava_vision_pair_stream", "gava_struct_sizes", "gava_clip_geometry_box",
           "gava_preprocess_clips", "gava_clip_geometry_view", "gava_view_scores",
           "gava_train_criterion", "gava_train_criterion_backward", "gava_train_head", "gava_train_head_backward",
           "gava_train_struct_sizes",
           "gava_nte_head", "gava_nte_head_backward", "gava_memory_head", "gava_memory_head_backward",
           "gava_memory_head_backward_workspace_floats", "gava_nte_head_backward_workspace_floats",
           "gava_sigmoid_criterion", "gava_sigmoid_criterion_backward", "gava_nte_diag_loss", "gava_nte_diag_loss_backward",
           "gava_aux_struct_sizes",
           "gava_adamw_plan", "gava_adamw_step", "gava_optim_struct_sizes",
           "gava_grad_norm", "gava_adamw_step_clipped", "gava_grad_clip_struct_sizes",
           "gava_unpatchify", "gava_input_grad_struct_sizes",
           "gava_attention_mass", "gava_attention_maps_struct_sizes",
           "gava_attention_relevance", "gava_attention_relevance_struct_sizes",
           "gava_patch_ranks", "gava_blur_clips", "gava_perturb_clips", "gava_perturb_scores", "gava_perturbation_struct_sizes",
           "gava_path_clips", "gava_clip_range", "gava_unpatchify_path", "gava_path_delta", "gava_path_grad_struct_sizes",
           "gava_mix_clips", "gava_mix_targets", "gava_soft_criterion", "gava_soft_criterion_backward", "gava_mix_struct_sizes",
           "gava_augment_hist", "gava_augment_luts", "gava_augment_apply", "gava_augment_struct_sizes"]
AUG_TABLE, AUG_COLOR, AUG_SHARPNESS, AUG_AFFINE = 0, 1, 2, 3      # gava_augment_desc.kind
AUG_INVERT, AUG_POSTERIZE, AUG_SOLARIZE, AUG_SOLARIZE_ADD, AUG_BRIGHTNESS, AUG_CONTRAST, AUG_AUTOCONTRAST, AUG_EQUALIZE = range(8)      # .op
AUG_BILINEAR, AUG_BICUBIC = 0, 1                                  # .filter
ATTENTION_MASS_MAX_KEYS = 640     # gava_attention_mass keeps K of one (frame, head) resident in LDS
ATTENTION_RELEVANCE_MAX_KEYS = 640     # and so does gava_attention_relevance
PERTURB_MAX_UNITS = 65536         # patches or frames one gava_patch_ranks ranking holds
PERTURB_MAX_STEPS = 128           # thresholds / fractions gava_perturb_clips and gava_perturb_scores take by value
BLUR_MAX_RADIUS = 64
RANK_PATCH, RANK_PIXEL, RANK_FRAME = 0, 1, 2
SCOPE_CLIP, SCOPE_FRAME = 0, 1
UNITS_PATCH, UNITS_FRAME = 0, 1
PERTURB_DELETION, PERTURB_INSERTION = 0, 1
BASELINE_ZERO, BASELINE_CHANNEL, BASELINE_TENSOR = 0, 1, 2
PATH_MAX_STEPS = 64               # copies of a clip gava_path_clips writes and gava_unpatchify_path reduces (alpha / w by value)
CLIP_RANGE_PARTS = 64             # workgroups per clip in gava_clip_range's first launch
PATH_LINE, PATH_NOISE = 0, 1      # gava_path_clips_args.mode
PATH_GRAD, PATH_ABSMAX, PATH_L2, PATH_ATTR, PATH_ATTR_SUM, PATH_ATTR_ABS = 0, 1, 2, 3, 4, 5      # gava_unpatchify_path_args.mode
ADAMW_MAX_GROUPS = 8

_vp, _fp, _ip = C.c_void_p, C.c_void_p, C.c_void_p  # all device pointers travel as void*


class GemmArgs(C.Structure):
    _fields_ = [("A", _vp), ("lda", C.c_int64), ("W", _vp), ("ldw", C.c_int64), ("bias", _fp),
                ("out", _vp), ("ldo", C.c_int64), ("resid", _fp), ("ldr", C.c_int64),
                ("M", C.c_int), ("N", C.c_int), ("K", C.c_int), ("epilogue", C.c_int), ("prec", C.c_int),
                ("scale_cols", C.c_int), ("scale", C.c_float),
                ("pos", _fp), ("time", _fp), ("n_patches", C.c_int), ("T", C.c_int),
                ("frames", _fp), ("frame_size", C.c_int), ("patch", C.c_int), ("split_out", C.c_int),
                ("aux", _vp), ("aux_prec", C.c_int), ("aux_out", _vp),
                ("x16_out", _vp), ("ld_x16", C.c_int64), ("rowsum_out", _fp),
                ("fold_stats", _fp), ("fold_s", _fp), ("fold_t", _fp), ("cu_reserve", C.c_int),
                ("rowsum_reduced", C.c_int), ("fold_partials", _fp),
                ("clips", _vp), ("clip_lut", _fp), ("kernel", C.c_int),
                ("w_lo", C.c_int), ("A8", _vp), ("lda8", C.c_int64), ("W8", _vp), ("ldw8", C.c_int64), ("w8_exp", C.c_int),
                ("out8", _vp), ("ldo8", C.c_int64), ("x8_out", _vp), ("ld_x8", C.c_int64),
                ("resid16", _vp), ("resid_lo", _vp), ("xlo_out", _vp)]


class LayerNormArgs(C.Structure):
    _fields_ = [("inp", _fp), ("in_stride", C.c_int64), ("in_row_index", _ip), ("gamma", _fp), ("beta", _fp),
                ("out16", _vp), ("out16_stride", C.c_int64), ("out32", _fp), ("out32_stride", C.c_int64),
                ("rows", C.c_int), ("D", C.c_int), ("prec", C.c_int), ("split_out", C.c_int),
                ("gamma2", _fp), ("beta2", _fp),
                ("out_hi", _vp), ("out_lo", _vp), ("out_hl_stride", C.c_int64)]


class AttentionArgs(C.Structure):
    _fields_ = [("q", _vp), ("k", _vp), ("v", _vp), ("ld_qkv", C.c_int64),
                ("side_k", _vp), ("side_v", _vp), ("ld_side", C.c_int64),
                ("out", _vp), ("ld_out", C.c_int64),
                ("batch", C.c_int), ("heads", C.c_int), ("n_q", C.c_int), ("n_kmain", C.c_int),
                ("n_g", C.c_int), ("T", C.c_int), ("has_summary", C.c_int),
                ("causal", C.c_int), ("prec", C.c_int), ("split_out", C.c_int),
                ("q_batch_rows", C.c_int), ("ld_q", C.c_int64)]


class ClipDesc(C.Structure):
    _fields_ = [("frames", _vp), ("n_frames", C.c_int), ("height", C.c_int), ("width", C.c_int),
                ("t_st", C.c_int), ("rate", C.c_int), ("h_st", C.c_int), ("w_st", C.c_int),
                ("scale_h", C.c_float), ("scale_w", C.c_float),
                ("box_y", C.c_int), ("box_x", C.c_int), ("box_h", C.c_int), ("box_w", C.c_int), ("lerp4_frames", C.c_int),
                ("frame_idx", _ip)]


class VisionLayer(C.Structure):
    _fields_ = [(n, _vp) for n in (
        "w_qkv", "b_qkv", "w_out", "b_out", "w_fc1", "b_fc1", "w_fc2", "b_fc2",
        "ln1_g", "ln1_b", "ln2_g", "ln2_b", "w_cls", "b_cls", "sln_g", "sln_b",
        "w_sqkv", "b_sqkv", "w_sout", "b_sout", "local_prompts", "global_prompts",
        "w_qkv_fold", "qkv_fold_s", "qkv_fold_t", "w_fc1_fold", "fc1_fold_s", "fc1_fold_t",
        "w_q_split", "w_out_split", "w_fc1_split", "w_fc2_split")]


class VisionModel(C.Structure):
    _fields_ = [("B", C.c_int), ("T_in", C.c_int), ("T_model", C.c_int),
                ("size", C.c_int), ("P", C.c_int), ("D", C.c_int), ("H", C.c_int), ("layers", C.c_int),
                ("F", C.c_int), ("E", C.c_int), ("G", C.c_int), ("prec", C.c_int),
                ("w_patch", _vp), ("b_patch", _fp), ("cls_token", _fp), ("pos_embed", _fp), ("time_embed", _fp),
                ("lnpre_g", _fp), ("lnpre_b", _fp), ("lnpost_g", _fp), ("lnpost_b", _fp),
                ("w_proj", _vp), ("layer", C.POINTER(VisionLayer)),
                ("clips", _vp), ("clip_lut", _fp), ("w_lo", C.c_int), ("layer8", _vp)]


class VisionLayer8(C.Structure):
    _fields_ = [(n, _vp) for n in ("w_qkv_fold8", "w_fc1_fold8", "w_fc28", "qkv_fold_s8", "fc1_fold_s8")] + \
               [(n, C.c_int) for n in ("qkv_fold_exp", "fc1_fold_exp", "fc2_exp")]


class TextLayer(C.Structure):
    _fields_ = [(n, _vp) for n in (
        "w_qkv", "b_qkv", "w_out", "b_out", "w_fc", "b_fc", "w_proj", "b_proj",
        "ln1_g", "ln1_b", "ln2_g", "ln2_b")]


class AttentionF32Args(C.Structure):
    _fields_ = [("q", _fp), ("k", _fp), ("v", _fp), ("ld", C.c_int64), ("out", _vp), ("ld_out", C.c_int64),
                ("batch", C.c_int), ("heads", C.c_int), ("L", C.c_int), ("causal", C.c_int), ("prec", C.c_int),
                ("split_out", C.c_int), ("scale", C.c_float)]


class TextModel(C.Structure):
    _fields_ = [("n_prompts", C.c_int), ("L", C.c_int), ("W", C.c_int), ("H", C.c_int), ("layers", C.c_int),
                ("E", C.c_int), ("n_ctx", C.c_int), ("prec", C.c_int), ("split", C.c_int), ("attn_f32", C.c_int),
                ("token_embedding", _fp), ("positional_embedding", _fp), ("lnf_g", _fp), ("lnf_b", _fp),
                ("w_tproj", _vp), ("layer", C.POINTER(TextLayer))]


class PreprocessArgs(C.Structure):
    _fields_ = [("frames", _vp), ("n_frames", C.c_int), ("height", C.c_int), ("width", C.c_int),
                ("mean", C.c_float * 3), ("std", C.c_float * 3),
                ("T", C.c_int), ("rate", C.c_int), ("size", C.c_int),
                ("out", _fp), ("out_stride_c", C.c_int64), ("out_stride_t", C.c_int64),
                ("first_temporal_view", C.c_int), ("first_spatial_view", C.c_int), ("lut", _fp)]


class PreprocessClipsArgs(C.Structure):
    _fields_ = [("clips", _vp), ("lut", _fp), ("B", C.c_int), ("T", C.c_int), ("size", C.c_int),
                ("out", _fp), ("out_stride_b", C.c_int64), ("out_stride_c", C.c_int64), ("out_stride_t", C.c_int64)]


class ViewScoresArgs(C.Structure):
    _fields_ = [("logits", _fp), ("ld_video", C.c_int64), ("ld_view", C.c_int64),
                ("B", C.c_int), ("V", C.c_int), ("C", C.c_int), ("scores", _fp), ("top1", _ip)]


class TrainCriterionArgs(C.Structure):
    _fields_ = [("logits", _fp), ("ld_logits", C.c_int64), ("labels", _ip),
                ("B", C.c_int), ("C", C.c_int), ("weighted", C.c_int),
                ("alpha", C.c_float), ("gamma", C.c_float), ("beta", C.c_float), ("scale", C.c_float),
                ("loss", _fp), ("per_sample", _fp), ("weight", _fp), ("top1", _ip), ("hits", _ip), ("conf", _ip),
                ("saved", _fp), ("grad_loss", _fp), ("dlogits", _fp), ("ld_dlogits", C.c_int64)]


class TrainHeadArgs(C.Structure):
    _fields_ = [("video", _fp), ("text", _fp), ("class_offsets", _ip), ("logit_scale", _fp), ("logit_bias", _fp),
                ("B", C.c_int), ("C", C.c_int), ("P", C.c_int), ("E", C.c_int),
                ("logits", _fp), ("text_features", _fp),
                ("video_norm", _fp), ("video_inv", _fp), ("text_norm", _fp), ("text_inv", _fp), ("class_mean", _fp),
                ("dlogits", _fp), ("dtext_features", _fp),
                ("dvideo", _fp), ("dtext", _fp), ("dlogit_scale", _fp), ("dlogit_bias", _fp), ("workspace", _fp)]


class NteHeadArgs(C.Structure):
    _fields_ = [("summary", _fp), ("weight", _fp), ("bias", _fp), ("video_nte", _fp), ("logit_scale", _fp),
                ("B", C.c_int), ("D", C.c_int), ("E", C.c_int), ("K", C.c_int),
                ("logits_vm", _fp),
                ("sp_norm", _fp), ("sp_inv", _fp), ("nte_mean", _fp), ("valid", _fp), ("sim", _fp), ("lm", _fp),
                ("row_lse", _fp), ("col_lse", _fp),
                ("dlogits", _fp), ("dsummary", _fp), ("dweight", _fp), ("dbias", _fp), ("dlogit_scale", _fp), ("workspace", _fp)]


class MemoryHeadArgs(C.Structure):
    _fields_ = [("memory", _fp), ("text_features", _fp), ("tf_w1", _fp), ("tf_b1", _fp), ("tf_w2", _fp), ("tf_b2", _fp),
                ("mem_params", _vp), ("logit_scale", _fp), ("logit_bias", _fp),
                ("M", C.c_int), ("S", C.c_int), ("C", C.c_int), ("E", C.c_int),
                ("logits_mt", _fp),
                ("mem_mean", _fp), ("mem_h", _fp), ("mem_z", _fp), ("mem_inv", _fp), ("tf_h", _fp), ("tf_u", _fp), ("tf_inv", _fp),
                ("cosine", _fp), ("lse", _fp),
                ("dlogits", _fp), ("dmem_w1", _fp), ("dmem_b1", _fp), ("dmem_w2", _fp), ("dmem_b2", _fp),
                ("dtf_w1", _fp), ("dtf_b1", _fp), ("dtf_w2", _fp), ("dtf_b2", _fp),
                ("dlogit_scale", _fp), ("dlogit_bias", _fp), ("dtext_features", _fp), ("workspace", _fp)]


class SigmoidCriterionArgs(C.Structure):
    _fields_ = [("logits", _fp), ("ld_logits", C.c_int64), ("labels", _ip),
                ("M", C.c_int), ("C", C.c_int), ("use_focal", C.c_int),
                ("alpha", C.c_float), ("gamma", C.c_float), ("scale", C.c_float),
                ("loss", _fp), ("per_sample", _fp), ("grad_loss", _fp), ("dlogits", _fp), ("ld_dlogits", C.c_int64)]


class NteDiagArgs(C.Structure):
    _fields_ = [("logits_vm", _fp), ("B", C.c_int), ("weight", C.c_float), ("loss", _fp), ("grad_loss", _fp), ("dlogits_vm", _fp)]


class AdamWTensor(C.Structure):
    _fields_ = [("p", _fp), ("g", _fp), ("m", _fp), ("v", _fp), ("step", _fp),
                ("copy_f32", _fp), ("copy16", _vp), ("copy_bf16", _vp), ("copy_bf16_t", _vp),
                ("ld_f32", C.c_int64), ("ld16", C.c_int64), ("ld_bf16", C.c_int64), ("ld_bf16_t", C.c_int64),
                ("n", C.c_int), ("group", C.c_int), ("rows", C.c_int), ("cols", C.c_int), ("prec16", C.c_int), ("reserved", C.c_int)]


class AdamWChunk(C.Structure):
    _fields_ = [("tensor", C.c_int), ("a", C.c_int), ("b", C.c_int), ("reserved", C.c_int)]


class AdamWGroup(C.Structure):
    _fields_ = [("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double), ("weight_decay", C.c_double)]


class AdamWArgs(C.Structure):
    _fields_ = [("table", _vp), ("table_host", C.POINTER(AdamWTensor)), ("chunks", _vp),
                ("n_tensors", C.c_int), ("n_chunks", C.c_int), ("n_groups", C.c_int), ("reserved", C.c_int),
                ("groups", AdamWGroup * 8), ("grad_scale", _fp), ("found_inf", _fp)]


class GradNormArgs(C.Structure):
    _fields_ = [("table", _vp), ("table_host", C.POINTER(AdamWTensor)), ("chunks", _vp),
                ("n_tensors", C.c_int), ("n_chunks", C.c_int), ("n_groups", C.c_int), ("reserved", C.c_int),
                ("grad_scale", _fp), ("max_norm", C.c_double), ("workspace", _vp), ("tensor_norm", _fp), ("stats", _fp)]


class PatchifyArgs(C.Structure):
    _fields_ = [("x", _fp), ("clips", _vp), ("clip_lut", _fp),
                ("B", C.c_int), ("T", C.c_int), ("size", C.c_int), ("patch", C.c_int), ("prec", C.c_int),
                ("out", _vp), ("ldo", C.c_int64)]


class UnpatchifyArgs(C.Structure):
    _fields_ = [("dpatch", _fp), ("ld", C.c_int64), ("x", _fp), ("out", _fp),
                ("B", C.c_int), ("T", C.c_int), ("size", C.c_int), ("patch", C.c_int), ("mode", C.c_int),
                ("frame_rows", C.c_int), ("row_offset", C.c_int), ("reserved", C.c_int)]


class AttentionMassArgs(C.Structure):
    _fields_ = [("q", _vp), ("k", _vp), ("ld_qkv", C.c_int64), ("side_k", _vp), ("ld_side", C.c_int64),
                ("w", _fp), ("out", _fp),
                ("batch", C.c_int), ("heads", C.c_int), ("n_q", C.c_int), ("n_kmain", C.c_int),
                ("n_g", C.c_int), ("T", C.c_int), ("has_summary", C.c_int), ("renorm", C.c_int), ("prec", C.c_int),
                ("q_batch_rows", C.c_int), ("ld_q", C.c_int64)]


class AttentionRelevanceArgs(C.Structure):
    _fields_ = [("q", _vp), ("k", _vp), ("v", _vp), ("ld_qkv", C.c_int64), ("side_k", _vp), ("ld_side", C.c_int64),
                ("dout", _vp), ("ld_dout", C.c_int64), ("w", _fp), ("out", _fp),
                ("batch", C.c_int), ("heads", C.c_int), ("n_q", C.c_int), ("n_kmain", C.c_int),
                ("n_g", C.c_int), ("T", C.c_int), ("has_summary", C.c_int),
                ("prec", C.c_int), ("act_prec_set", C.c_int), ("act_prec", C.c_int),
                ("q_batch_rows", C.c_int), ("reserved", C.c_int), ("ld_q", C.c_int64)]


class PatchRanksArgs(C.Structure):
    _fields_ = [("scores", _fp), ("ranks", _ip), ("pooled", _fp),
                ("B", C.c_int), ("T", C.c_int), ("g", C.c_int), ("patch", C.c_int), ("layout", C.c_int), ("scope", C.c_int)]


class BlurClipsArgs(C.Structure):
    _fields_ = [("x", _fp), ("taps", _fp), ("tmp", _fp), ("out", _fp),
                ("B", C.c_int), ("T", C.c_int), ("size", C.c_int), ("radius", C.c_int)]


class PerturbClipsArgs(C.Structure):
    _fields_ = [("x", _fp), ("ranks", _ip), ("baseline", _fp), ("out", _fp),
                ("nb", C.c_int), ("T", C.c_int), ("size", C.c_int), ("patch", C.c_int), ("units", C.c_int), ("mode", C.c_int),
                ("baseline_kind", C.c_int), ("n_steps", C.c_int), ("k", C.c_int * PERTURB_MAX_STEPS)]


class PerturbScoresArgs(C.Structure):
    _fields_ = [("logits", _fp), ("ld", C.c_int64), ("target", _ip), ("logit", _fp), ("prob", _fp), ("top1", _ip),
                ("auc_logit", _fp), ("auc_prob", _fp), ("target_out", _ip),
                ("nb", C.c_int), ("n_steps", C.c_int), ("C", C.c_int), ("ref_step", C.c_int),
                ("fractions", C.c_float * PERTURB_MAX_STEPS)]


class PathClipsArgs(C.Structure):
    _fields_ = [("x", _fp), ("baseline", _fp), ("sigma", _fp), ("out", _fp),
                ("nb", C.c_int), ("T", C.c_int), ("size", C.c_int), ("patch", C.c_int), ("mode", C.c_int),
                ("baseline_kind", C.c_int), ("m", C.c_int), ("clip0", C.c_int), ("seed", C.c_uint64),
                ("alpha", C.c_float * PATH_MAX_STEPS), ("beta", C.c_float * PATH_MAX_STEPS)]


class ClipRangeArgs(C.Structure):
    _fields_ = [("x", _fp), ("min", _fp), ("max", _fp), ("sigma", _fp), ("workspace", _fp),
                ("nb", C.c_int), ("T", C.c_int), ("size", C.c_int), ("rel", C.c_float)]


class UnpatchifyPathArgs(C.Structure):
    _fields_ = [("dpatch", _fp), ("ld", C.c_int64), ("x", _fp), ("baseline", _fp), ("out", _fp),
                ("B", C.c_int), ("T", C.c_int), ("size", C.c_int), ("patch", C.c_int), ("mode", C.c_int),
                ("baseline_kind", C.c_int), ("frame_rows", C.c_int), ("row_offset", C.c_int), ("m", C.c_int), ("reserved", C.c_int),
                ("w", C.c_float * PATH_MAX_STEPS)]


class PathDeltaArgs(C.Structure):
    _fields_ = [("map", _fp), ("logits", _fp), ("ld", C.c_int64), ("target", _ip),
                ("sum_attr", _fp), ("f_diff", _fp), ("delta", _fp),
                ("B", C.c_int), ("T", C.c_int), ("size", C.c_int), ("m", C.c_int), ("C", C.c_int),
                ("k_lo", C.c_int), ("k_hi", C.c_int), ("reserved", C.c_int)]


class MixDesc(C.Structure):
    _fields_ = [("partner", C.c_int32), ("lam", C.c_float), ("y0", C.c_int32), ("y1", C.c_int32), ("x0", C.c_int32), ("x1", C.c_int32)]


class MixClipsArgs(C.Structure):
    _fields_ = [("x", _fp), ("out", _fp), ("desc_host", C.c_void_p), ("desc", _vp),
                ("B", C.c_int), ("planes", C.c_int), ("H", C.c_int), ("W", C.c_int)]


class MixTargetsArgs(C.Structure):
    _fields_ = [("labels", _ip), ("desc", _vp), ("targets", _fp), ("ld_targets", C.c_int64),
                ("B", C.c_int), ("C", C.c_int), ("smoothing", C.c_float), ("reserved", C.c_int)]


class SoftCriterionArgs(C.Structure):
    _fields_ = [("logits", _fp), ("ld_logits", C.c_int64), ("targets", _fp), ("ld_targets", C.c_int64),
                ("B", C.c_int), ("C", C.c_int), ("weighted", C.c_int),
                ("alpha", C.c_float), ("gamma", C.c_float), ("beta", C.c_float), ("scale", C.c_float),
                ("loss", _fp), ("per_sample", _fp), ("weight", _fp), ("top1", _ip), ("target1", _ip), ("hits", _ip), ("conf", _ip),
                ("saved", _fp), ("grad_loss", _fp), ("dlogits", _fp), ("ld_dlogits", C.c_int64)]


class AugmentDesc(C.Structure):
    _fields_ = [("src", _vp), ("dst", _vp), ("H", C.c_int32), ("W", C.c_int32), ("kind", C.c_int32), ("op", C.c_int32),
                ("filter", C.c_int32), ("iarg", C.c_int32), ("factor", C.c_float), ("lut_slot", C.c_int32),
                ("hist_slot", C.c_int32), ("reserved", C.c_int32), ("m", C.c_double * 6)]


class AugmentArgs(C.Structure):
    _fields_ = [("desc_host", C.c_void_p), ("desc", _vp), ("hist", _vp), ("luts", _vp),
                ("n", C.c_int32), ("n_hist", C.c_int32), ("n_luts", C.c_int32), ("reserved", C.c_int32)]


class VisionSaved(C.Structure):
    _fields_ = [("e0", _fp), ("x", _fp), ("x1", _fp), ("qkv", _vp), ("pre", _vp), ("sidekv", _vp),
                ("last_q", _vp), ("last_x1", _fp), ("last_pre", _vp)]


class LayerNormBwdArgs(C.Structure):
    _fields_ = [("x", _fp), ("x_stride", C.c_int64), ("x_row_index", _ip), ("gamma", _fp),
                ("dy", _fp), ("dy_stride", C.c_int64),
                ("dx", _fp), ("dx_stride", C.c_int64), ("dx_row_index", _ip),
                ("dgamma", _fp), ("dbeta", _fp), ("rows", C.c_int), ("D", C.c_int), ("accumulate", C.c_int),
                ("dx16", _vp), ("dx16_stride", C.c_int64), ("prec", C.c_int)]


class AttentionBwdArgs(C.Structure):
    _fields_ = [("q", _vp), ("k", _vp), ("v", _vp), ("ld_qkv", C.c_int64), ("dout", _vp), ("ld_dout", C.c_int64),
                ("dq", _vp), ("dk", _vp), ("dv", _vp), ("ld_dqkv", C.c_int64),
                ("batch", C.c_int), ("heads", C.c_int), ("n", C.c_int), ("causal", C.c_int), ("prec", C.c_int),
                ("q_scale", C.c_float),
                ("side_k", _vp), ("side_v", _vp), ("ld_side", C.c_int64),
                ("dside_k", _fp), ("dside_v", _fp), ("ld_dside", C.c_int64),
                ("n_g", C.c_int), ("T", C.c_int), ("has_summary", C.c_int), ("n_q", C.c_int), ("workspace", _vp),
                ("act_prec_set", C.c_int), ("act_prec", C.c_int),
                ("q_batch_rows", C.c_int), ("ld_q", C.c_int64), ("ld_dq", C.c_int64)]


_lib = None


class GavaError(RuntimeError):
    pass


_ERR = {-1: "GAVA_EINVAL (unsupported shape/alignment)", -2: "GAVA_EWORKSPACE (workspace too small)",
        -3: "GAVA_ELAUNCH (kernel launch failed)"}


def load():
    """Load libgava_hip.so; raises GavaError when it has not been built (no CPU fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise GavaError(f"{LIB_PATH} is missing: run `python -m gava_clip_amd.build` "
                        "(the HIP path has no fallback)")
    lib = C.CDLL(LIB_PATH)
    lib.gava_abi_version.restype = C.c_int
    # the library reports the hash of the header it was compiled against; the ctypes mirrors in this file follow the header
    # in the tree (tests/test_host_cpu.py compares every struct size with the C compiler's): a stale .so would be called with
    # shifted structs, so it is refused here
    from .build import abi_hash, HEADER
    try:
        want = abi_hash()
    except OSError as e:
        raise GavaError(f"cannot read {os.path.normpath(HEADER)} ({e}): the ctypes mirrors in gava_clip_amd/hip.py are checked against "
                        "the ABI hash of that header, keep include/gava_hip.h next to the package") from None
    have = lib.gava_abi_version()
    if have != want:
        raise GavaError(f"{LIB_PATH} was built from another include/gava_hip.h (ABI {have:#x}, header in the tree {want:#x}): "
                        "rebuild with `python -m gava_clip_amd.build --force`")
    for name, args in (("gava_gemm", [C.POINTER(GemmArgs), _vp]),
                       ("gava_layernorm", [C.POINTER(LayerNormArgs), _vp]),
                       ("gava_attention", [C.POINTER(AttentionArgs), _vp])):
        f = getattr(lib, name)
        f.argtypes, f.restype = args, C.c_int
    lib.gava_attention_f32.argtypes, lib.gava_attention_f32.restype = [C.POINTER(AttentionF32Args), _vp], C.c_int
    lib.gava_vision_workspace_bytes.argtypes = [C.POINTER(VisionModel)]
    lib.gava_vision_workspace_bytes.restype = C.c_size_t
    lib.gava_vision_forward.argtypes = [C.POINTER(VisionModel), _fp, _fp, _fp, _fp, _vp, C.c_size_t, _vp]
    lib.gava_vision_forward.restype = C.c_int
    lib.gava_text_workspace_bytes.argtypes = [C.POINTER(TextModel)]
    lib.gava_text_workspace_bytes.restype = C.c_size_t
    lib.gava_text_forward.argtypes = [C.POINTER(TextModel), _ip, _fp, _ip, _fp, _vp, C.c_size_t, _vp]
    lib.gava_text_forward.restype = C.c_int
    lib.gava_similarity_head.argtypes = [_fp, _fp, _fp, _fp, C.c_int, C.c_int, C.c_int, C.c_int, _fp, _fp, _fp, _vp]
    lib.gava_similarity_head.restype = C.c_int
    lib.gava_convert_h16.argtypes = [_fp, _vp, C.c_size_t, C.c_int, _vp]
    lib.gava_convert_h16.restype = C.c_int
    lib.gava_preprocess_clip.argtypes = [C.POINTER(PreprocessArgs), _vp]
    lib.gava_preprocess_clip.restype = C.c_int
    lib.gava_patchify.argtypes = [C.POINTER(PatchifyArgs), _vp]
    lib.gava_patchify.restype = C.c_int
    lib.gava_layernorm_backward.argtypes = [C.POINTER(LayerNormBwdArgs), _vp]
    lib.gava_layernorm_backward.restype = C.c_int
    lib.gava_qgelu_backward.argtypes = [_vp, _vp, _vp, C.c_size_t, C.c_int, _vp]
    lib.gava_qgelu_backward.restype = C.c_int
    lib.gava_attention_backward.argtypes = [C.POINTER(AttentionBwdArgs), _vp]
    lib.gava_attention_backward.restype = C.c_int
    lib.gava_attention_backward_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
    lib.gava_attention_backward_workspace_bytes.restype = C.c_size_t
    lib.gava_clip_geometry.argtypes = [C.POINTER(ClipDesc), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.gava_clip_geometry.restype = C.c_int
    lib.gava_clip_geometry_box.argtypes = [C.POINTER(ClipDesc), C.c_int, C.c_int, C.POINTER(C.c_int), _ip] + [C.c_int] * 4
    lib.gava_clip_geometry_box.restype = C.c_int
    lib.gava_preprocess_clips.argtypes, lib.gava_preprocess_clips.restype = [C.POINTER(PreprocessClipsArgs), _vp], C.c_int
    lib.gava_clip_geometry_view.argtypes, lib.gava_clip_geometry_view.restype = [C.POINTER(ClipDesc)] + [C.c_int] * 6, C.c_int
    lib.gava_view_scores.argtypes, lib.gava_view_scores.restype = [C.POINTER(ViewScoresArgs), _vp], C.c_int
    lib.gava_gemm_aligned_walk.argtypes, lib.gava_gemm_aligned_walk.restype = [C.c_int, C.c_int, C.c_int], C.c_int
    lib.gava_probe_fc1_enable.argtypes = [C.c_int]
    lib.gava_probe_fc1_read.argtypes = [C.POINTER(C.c_float), C.c_int]
    lib.gava_row_stats.argtypes = [_fp, C.c_int, C.c_int, C.c_int, _fp, _vp]
    lib.gava_row_stats.restype = C.c_int
    lib.gava_vision_forward_keep.argtypes = [C.POINTER(VisionModel), _fp, _fp, _fp, C.POINTER(VisionSaved), _vp, C.c_size_t, _vp]
    lib.gava_vision_forward_keep.restype = C.c_int
    lib.gava_vision_forward_train.argtypes = [C.POINTER(VisionModel), _fp, _fp, _fp, _fp, _fp, _vp, C.c_size_t, _vp]
    lib.gava_vision_forward_train.restype = C.c_int
    lib.gava_text_forward_train.argtypes = [C.POINTER(TextModel), _ip, _fp, _ip, _fp, _fp, _vp, C.c_size_t, _vp]
    lib.gava_text_forward_train.restype = C.c_int
    lib.gava_vision_pair_stream.argtypes, lib.gava_vision_pair_stream.restype = [C.POINTER(VisionModel)], C.c_int
    # the header the library was compiled from against the mirrors above (gava_abi_version ties library and header)
    mirrors = [GemmArgs, LayerNormArgs, AttentionArgs, AttentionF32Args, ClipDesc, VisionLayer, VisionLayer8, VisionModel, TextLayer,
               TextModel, LayerNormBwdArgs, AttentionBwdArgs, VisionSaved, PreprocessArgs, PatchifyArgs, PreprocessClipsArgs,
               ViewScoresArgs]
    sizes = (C.c_size_t * len(mirrors))()
    lib.gava_struct_sizes.argtypes, lib.gava_struct_sizes.restype = [C.POINTER(C.c_size_t), C.c_int], C.c_int
    if lib.gava_struct_sizes(sizes, len(mirrors)) != len(mirrors):
        raise GavaError("libgava_hip.so and gava_clip_amd/hip.py disagree on the number of ABI structs")
    for cls, sz in zip(mirrors, sizes):
        if C.sizeof(cls) != sz:
            raise GavaError(f"ctypes mirror {cls.__name__} is {C.sizeof(cls)} bytes, the library's struct {sz}: gava_clip_amd/hip.py is out of "
                            f"step with include/gava_hip.h")
    # the training head's structs report through their own call (gava_struct_sizes keeps its list)
    for name in ("gava_train_criterion", "gava_train_criterion_backward"):
        getattr(lib, name).argtypes, getattr(lib, name).restype = [C.POINTER(TrainCriterionArgs), _vp], C.c_int
    for name in ("gava_train_head", "gava_train_head_backward"):
        getattr(lib, name).argtypes, getattr(lib, name).restype = [C.POINTER(TrainHeadArgs), _vp], C.c_int
    train_mirrors = [TrainCriterionArgs, TrainHeadArgs]
    lib.gava_train_struct_sizes.argtypes, lib.gava_train_struct_sizes.restype = [C.POINTER(C.c_size_t), C.c_int], C.c_int
    if lib.gava_train_struct_sizes(sizes, len(train_mirrors)) != len(train_mirrors):
        raise GavaError("libgava_hip.so and gava_clip_amd/hip.py disagree on the number of training-head ABI structs")
    for cls, sz in zip(train_mirrors, sizes):
        if C.sizeof(cls) != sz:
            raise GavaError(f"ctypes mirror {cls.__name__} is {C.sizeof(cls)} bytes, the library's struct {sz}: gava_clip_amd/hip.py is out of "
                            f"step with include/gava_hip.h")
    # the auxiliary heads' structs, the same way
    aux_mirrors = [NteHeadArgs, MemoryHeadArgs, SigmoidCriterionArgs, NteDiagArgs]
    for names, cls in ((("gava_nte_head", "gava_nte_head_backward"), NteHeadArgs),
                       (("gava_memory_head", "gava_memory_head_backward"), MemoryHeadArgs),
                       (("gava_sigmoid_criterion", "gava_sigmoid_criterion_backward"), SigmoidCriterionArgs),
                       (("gava_nte_diag_loss", "gava_nte_diag_loss_backward"), NteDiagArgs)):
        for name in names:
            getattr(lib, name).argtypes, getattr(lib, name).restype = [C.POINTER(cls), _vp], C.c_int
    lib.gava_nte_head_backward_workspace_floats.argtypes = [C.c_int, C.c_int]
    lib.gava_nte_head_backward_workspace_floats.restype = C.c_size_t
    lib.gava_memory_head_backward_workspace_floats.argtypes = [C.c_int, C.c_int, C.c_int]
    lib.gava_memory_head_backward_workspace_floats.restype = C.c_size_t
    lib.gava_aux_struct_sizes.argtypes, lib.gava_aux_struct_sizes.restype = [C.POINTER(C.c_size_t), C.c_int], C.c_int
    if lib.gava_aux_struct_sizes(sizes, len(aux_mirrors)) != len(aux_mirrors):
        raise GavaError("libgava_hip.so and gava_clip_amd/hip.py disagree on the number of auxiliary-head ABI structs")
    for cls, sz in zip(aux_mirrors, sizes):
        if C.sizeof(cls) != sz:
            raise GavaError(f"ctypes mirror {cls.__name__} is {C.sizeof(cls)} bytes, the library's struct {sz}: gava_clip_amd/hip.py is out of "
                            f"step with include/gava_hip.h")
    # the fused optimizer's structs, the same way
    optim_mirrors = [AdamWTensor, AdamWArgs, AdamWChunk]
    lib.gava_adamw_plan.argtypes = [C.POINTER(AdamWTensor), C.c_int, C.c_int, C.POINTER(AdamWChunk), C.c_int]
    lib.gava_adamw_plan.restype = C.c_int
    lib.gava_adamw_step.argtypes, lib.gava_adamw_step.restype = [C.POINTER(AdamWArgs), _vp], C.c_int
    lib.gava_optim_struct_sizes.argtypes, lib.gava_optim_struct_sizes.restype = [C.POINTER(C.c_size_t), C.c_int], C.c_int
    if lib.gava_optim_struct_sizes(sizes, len(optim_mirrors)) != len(optim_mirrors):
        raise GavaError("libgava_hip.so and gava_clip_amd/hip.py disagree on the number of optimizer ABI structs")
    for cls, sz in zip(optim_mirrors, sizes):
        if C.sizeof(cls) != sz:
            raise GavaError(f"ctypes mirror {cls.__name__} is {C.sizeof(cls)} bytes, the library's struct {sz}: gava_clip_amd/hip.py is out of "
                            f"step with include/gava_hip.h")
    # the gradient clip's struct, the same way
    grad_clip_mirrors = [GradNormArgs]
    lib.gava_grad_norm.argtypes, lib.gava_grad_norm.restype = [C.POINTER(GradNormArgs), _vp], C.c_int
    lib.gava_adamw_step_clipped.argtypes, lib.gava_adamw_step_clipped.restype = [C.POINTER(AdamWArgs), _fp, _vp], C.c_int
    lib.gava_grad_clip_struct_sizes.argtypes, lib.gava_grad_clip_struct_sizes.restype = [C.POINTER(C.c_size_t), C.c_int], C.c_int
    if lib.gava_grad_clip_struct_sizes(sizes, len(grad_clip_mirrors)) != len(grad_clip_mirrors):
        raise GavaError("libgava_hip.so and gava_clip_amd/hip.py disagree on the number of gradient-clip ABI structs")
    for cls, sz in zip(grad_clip_mirrors, sizes):
        if C.sizeof(cls) != sz:
            raise GavaError(f"ctypes mirror {cls.__name__} is {C.sizeof(cls)} bytes, the library's struct {sz}: gava_clip_amd/hip.py is out of "
                            f"step with include/gava_hip.h")
    # the input gradient's struct, the same way
    input_grad_mirrors = [UnpatchifyArgs]
    lib.gava_unpatchify.argtypes, lib.gava_unpatchify.restype = [C.POINTER(UnpatchifyArgs), _vp], C.c_int
    lib.gava_input_grad_struct_sizes.argtypes, lib.gava_input_grad_struct_sizes.restype = [C.POINTER(C.c_size_t), C.c_int], C.c_int
    if lib.gava_input_grad_struct_sizes(sizes, len(input_grad_mirrors)) != len(input_grad_mirrors):
        raise GavaError("libgava_hip.so and gava_clip_amd/hip.py disagree on the number of input-gradient ABI structs")
    for cls, sz in zip(input_grad_mirrors, sizes):
        if C.sizeof(cls) != sz:
            raise GavaError(f"ctypes mirror {cls.__name__} is {C.sizeof(cls)} bytes, the library's struct {sz}: gava_clip_amd/hip.py is out of "
                            f"step with include/gava_hip.h")
    # the attention maps' struct, the same way
    maps_mirrors = [AttentionMassArgs]
    lib.gava_attention_mass.argtypes, lib.gava_attention_mass.restype = [C.POINTER(AttentionMassArgs), _vp], C.c_int
    lib.gava_attention_maps_struct_sizes.argtypes, lib.gava_attention_maps_struct_sizes.restype = [C.POINTER(C.c_size_t), C.c_int], C.c_int
    if lib.gava_attention_maps_struct_sizes(sizes, len(maps_mirrors)) != len(maps_mirrors):
        raise GavaError("libgava_hip.so and gava_clip_amd/hip.py disagree on the number of attention-map ABI structs")
    for cls, sz in zip(maps_mirrors, sizes):
        if C.sizeof(cls) != sz:
            raise GavaError(f"ctypes mirror {cls.__name__} is {C.sizeof(cls)} bytes, the library's struct {sz}: gava_clip_amd/hip.py is out of "
                            f"step with include/gava_hip.h")
    # the relevance step's struct, the same way
    relevance_mirrors = [AttentionRelevanceArgs]
    lib.gava_attention_relevance.argtypes, lib.gava_attention_relevance.restype = [C.POINTER(AttentionRelevanceArgs), _vp], C.c_int
    lib.gava_attention_relevance_struct_sizes.argtypes, lib.gava_attention_relevance_struct_sizes.restype = [C.POINTER(C.c_size_t), C.c_int], C.c_int
    if lib.gava_attention_relevance_struct_sizes(sizes, len(relevance_mirrors)) != len(relevance_mirrors):
        raise GavaError("libgava_hip.so and gava_clip_amd/hip.py disagree on the number of relevance ABI structs")
    for cls, sz in zip(relevance_mirrors, sizes):
        if C.sizeof(cls) != sz:
            raise GavaError(f"ctypes mirror {cls.__name__} is {C.sizeof(cls)} bytes, the library's struct {sz}: gava_clip_amd/hip.py is out of "
                            f"step with include/gava_hip.h")
    # the faithfulness curves' structs, the same way
    perturbation_mirrors = [PatchRanksArgs, BlurClipsArgs, PerturbClipsArgs, PerturbScoresArgs]
    for name, cls in (("gava_patch_ranks", PatchRanksArgs), ("gava_blur_clips", BlurClipsArgs),
                      ("gava_perturb_clips", PerturbClipsArgs), ("gava_perturb_scores", PerturbScoresArgs)):
        getattr(lib, name).argtypes, getattr(lib, name).restype = [C.POINTER(cls), _vp], C.c_int
    lib.gava_perturbation_struct_sizes.argtypes, lib.gava_perturbation_struct_sizes.restype = [C.POINTER(C.c_size_t), C.c_int], C.c_int
    if lib.gava_perturbation_struct_sizes(sizes, len(perturbation_mirrors)) != len(perturbation_mirrors):
        raise GavaError("libgava_hip.so and gava_clip_amd/hip.py disagree on the number of perturbation ABI structs")
    for cls, sz in zip(perturbation_mirrors, sizes):
        if C.sizeof(cls) != sz:
            raise GavaError(f"ctypes mirror {cls.__name__} is {C.sizeof(cls)} bytes, the library's struct {sz}: gava_clip_amd/hip.py is out of "
                            f"step with include/gava_hip.h")
    # the path gradients' structs, the same way
    path_mirrors = [PathClipsArgs, ClipRangeArgs, UnpatchifyPathArgs, PathDeltaArgs]
    for name, cls in (("gava_path_clips", PathClipsArgs), ("gava_clip_range", ClipRangeArgs),
                      ("gava_unpatchify_path", UnpatchifyPathArgs), ("gava_path_delta", PathDeltaArgs)):
        getattr(lib, name).argtypes, getattr(lib, name).restype = [C.POINTER(cls), _vp], C.c_int
    lib.gava_path_grad_struct_sizes.argtypes, lib.gava_path_grad_struct_sizes.restype = [C.POINTER(C.c_size_t), C.c_int], C.c_int
    if lib.gava_path_grad_struct_sizes(sizes, len(path_mirrors)) != len(path_mirrors):
        raise GavaError("libgava_hip.so and gava_clip_amd/hip.py disagree on the number of path-gradient ABI structs")
    for cls, sz in zip(path_mirrors, sizes):
        if C.sizeof(cls) != sz:
            raise GavaError(f"ctypes mirror {cls.__name__} is {C.sizeof(cls)} bytes, the library's struct {sz}: gava_clip_amd/hip.py is out of "
                            f"step with include/gava_hip.h")
    # the mix's and the soft-target criterion's structs, the same way
    mix_mirrors = [MixDesc, MixClipsArgs, MixTargetsArgs, SoftCriterionArgs]
    for name, cls in (("gava_mix_clips", MixClipsArgs), ("gava_mix_targets", MixTargetsArgs),
                      ("gava_soft_criterion", SoftCriterionArgs), ("gava_soft_criterion_backward", SoftCriterionArgs)):
        getattr(lib, name).argtypes, getattr(lib, name).restype = [C.POINTER(cls), _vp], C.c_int
    lib.gava_mix_struct_sizes.argtypes, lib.gava_mix_struct_sizes.restype = [C.POINTER(C.c_size_t), C.c_int], C.c_int
    if lib.gava_mix_struct_sizes(sizes, len(mix_mirrors)) != len(mix_mirrors):
        raise GavaError("libgava_hip.so and gava_clip_amd/hip.py disagree on the number of mix ABI structs")
    for cls, sz in zip(mix_mirrors, sizes):
        if C.sizeof(cls) != sz:
            raise GavaError(f"ctypes mirror {cls.__name__} is {C.sizeof(cls)} bytes, the library's struct {sz}: gava_clip_amd/hip.py is out of "
                            f"step with include/gava_hip.h")
    # the augmentation's structs, the same way
    augment_mirrors = [AugmentDesc, AugmentArgs]
    for name in ("gava_augment_hist", "gava_augment_luts", "gava_augment_apply"):
        getattr(lib, name).argtypes, getattr(lib, name).restype = [C.POINTER(AugmentArgs), _vp], C.c_int
    lib.gava_augment_struct_sizes.argtypes, lib.gava_augment_struct_sizes.restype = [C.POINTER(C.c_size_t), C.c_int], C.c_int
    if lib.gava_augment_struct_sizes(sizes, len(augment_mirrors)) != len(augment_mirrors):
        raise GavaError("libgava_hip.so and gava_clip_amd/hip.py disagree on the number of augmentation ABI structs")
    for cls, sz in zip(augment_mirrors, sizes):
        if C.sizeof(cls) != sz:
            raise GavaError(f"ctypes mirror {cls.__name__} is {C.sizeof(cls)} bytes, the library's struct {sz}: gava_clip_amd/hip.py is out of "
                            f"step with include/gava_hip.h")
    _lib = lib
    return lib


def check(code, what):
    if code != 0:
        raise GavaError(f"{what} failed: {_ERR.get(code, code)}")


def stream_ptr(device=None):
    """torch's current HIP stream on `device` (default: the current device).  The drivers key their per-device launch
    context by the CURRENT device, so callers that may be handed a tensor of another device wrap the call in
    `torch.cuda.device(t.device)` (model.py does)."""
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def ptr(t):
    """Device pointer of a CUDA/HIP tensor (None -> NULL)."""
    if t is None:
        return None
    assert t.is_cuda, "gava_clip_amd kernels take device tensors only"
    return C.c_void_p(t.data_ptr())


def h16_dtype(prec):
    return PREC_TORCH[prec]


# ---- thin per-op wrappers (used by the unit tests; the model uses the fused drivers) ----------

def gemm(A, W, bias, out, *, epilogue, prec, resid=None, scale_cols=0, scale=1.0,
         pos=None, time=None, n_patches=0, T=0, M=None, split_out=False, frames=None, frame_size=0, patch=0, aux=None,
         aux_prec=None, aux_out=None, x16_out=None, rowsum_out=None, fold_stats=None, fold_s=None, fold_t=None,
         cu_reserve=0, rowsum_reduced=False, fold_partials=None, clips=None, clip_lut=None, kernel=0, w_lo=0, K=None,
         A8=None, W8=None, w8_exp=0, out8=None, x8_out=None, resid16=None, resid_lo=None, xlo_out=None):
    a = GemmArgs()
    a.resid16, a.resid_lo, a.xlo_out = ptr(resid16), ptr(resid_lo), ptr(xlo_out)
    a.kernel = kernel
    a.w_lo, a.w8_exp = w_lo, w8_exp
    a.A8, a.lda8, a.W8, a.ldw8 = ptr(A8), (A8.stride(0) if A8 is not None else 0), ptr(W8), (W8.stride(0) if W8 is not None else 0)
    a.out8, a.ldo8 = ptr(out8), (out8.stride(0) if out8 is not None else 0)
    a.x8_out, a.ld_x8 = ptr(x8_out), (x8_out.stride(0) if x8_out is not None else 0)
    a.clips, a.clip_lut = ptr(clips), ptr(clip_lut)
    a.cu_reserve = cu_reserve
    a.rowsum_reduced, a.fold_partials = int(rowsum_reduced), ptr(fold_partials)
    a.x16_out, a.ld_x16, a.rowsum_out = ptr(x16_out), (x16_out.stride(0) if x16_out is not None else 0), ptr(rowsum_out)
    a.fold_stats, a.fold_s, a.fold_t = ptr(fold_stats), ptr(fold_s), ptr(fold_t)
    a.aux, a.aux_out = ptr(aux), ptr(aux_out)
    a.aux_prec = prec if aux_prec is None else aux_prec
    a.A, a.lda, a.W, a.ldw = ptr(A), (A.stride(0) if A is not None else W.stride(0)), ptr(W), W.stride(0)
    a.frames, a.frame_size, a.patch = ptr(frames), frame_size, patch
    a.bias, a.out, a.ldo = ptr(bias), ptr(out), (out.stride(0) if out is not None else 0)
    a.resid, a.ldr = ptr(resid), (resid.stride(0) if resid is not None else (resid16.stride(0) if resid16 is not None else 0))
    a.M, a.N, a.K = (A.shape[0] if M is None else M), W.shape[0], (W.shape[1] // (2 if w_lo == 1 else 1) if K is None else K)
    a.epilogue, a.prec, a.scale_cols, a.scale = epilogue, prec, scale_cols, scale
    a.pos, a.time, a.n_patches, a.T = ptr(pos), ptr(time), n_patches, T
    a.split_out = int(split_out)
    check(load().gava_gemm(C.byref(a), stream_ptr()), "gava_gemm")


def attention_f32(q, k, v, out, *, batch, heads, L, prec, causal=False, split_out=False, scale=0.125):
    a = AttentionF32Args()
    a.q, a.k, a.v, a.ld = ptr(q), ptr(k), ptr(v), q.stride(0)
    a.out, a.ld_out = ptr(out), out.stride(0)
    a.batch, a.heads, a.L, a.causal, a.prec, a.split_out, a.scale = batch, heads, L, int(causal), prec, int(split_out), scale
    check(load().gava_attention_f32(C.byref(a), stream_ptr()), "gava_attention_f32")


def layernorm(x, gamma, beta, *, out16=None, out32=None, prec, rows=None, in_stride=None, row_index=None,
              split_out=False, gamma2=None, beta2=None, out_hi=None, out_lo=None):
    a = LayerNormArgs()
    a.out_hi, a.out_lo, a.out_hl_stride = ptr(out_hi), ptr(out_lo), (out_hi.stride(0) if out_hi is not None else 0)
    a.gamma2, a.beta2 = ptr(gamma2), ptr(beta2)
    a.inp, a.in_stride, a.in_row_index = ptr(x), (x.stride(0) if in_stride is None else in_stride), ptr(row_index)
    a.gamma, a.beta = ptr(gamma), ptr(beta)
    a.out16, a.out16_stride = ptr(out16), (out16.stride(0) if out16 is not None else 0)
    a.out32, a.out32_stride = ptr(out32), (out32.stride(0) if out32 is not None else 0)
    a.rows, a.D, a.prec = (x.shape[0] if rows is None else rows), x.shape[-1], prec
    a.split_out = int(split_out)
    check(load().gava_layernorm(C.byref(a), stream_ptr()), "gava_layernorm")


def attention(q, k, v, out, *, batch, heads, n_q, n_kmain, prec, causal=False,
              side_k=None, side_v=None, n_g=0, T=0, has_summary=False, split_out=False, q_batch_rows=0):
    a = AttentionArgs()
    a.q, a.k, a.v, a.ld_qkv = ptr(q), ptr(k), ptr(v), k.stride(0)   # q may be a separate buffer (q_batch_rows, ld_q)
    a.side_k, a.side_v = ptr(side_k), ptr(side_v)
    a.ld_side = side_k.stride(0) if side_k is not None else 0
    a.out, a.ld_out = ptr(out), out.stride(0)
    a.batch, a.heads, a.n_q, a.n_kmain = batch, heads, n_q, n_kmain
    a.n_g, a.T, a.has_summary, a.causal, a.prec = n_g, T, int(has_summary), int(causal), prec
    a.split_out = int(split_out)
    a.q_batch_rows, a.ld_q = q_batch_rows, (q.stride(0) if q_batch_rows else 0)
    check(load().gava_attention(C.byref(a), stream_ptr()), "gava_attention")


def split_pack_weight(w, prec):
    """[N][K] fp32 -> [N][3K] h16 = [W_hi | W_hi | W_lo], the weight side of the split-precision GEMM."""
    w = w.detach().float().contiguous()
    hi = convert_h16(w, prec)
    lo = convert_h16(w - hi.float(), prec)
    return torch.cat([hi, hi, lo], dim=1).contiguous()


def pack_w8(w, prec):
    """The 8-bit lo operand of a weight (gava_gemm_args.w_lo = 2): (hi16, W8, exp, row sums) with hi16 = h16(w), W8 = e4m3 bytes
    of 2^exp (w - hi16) in rows 4K bytes apart (K used), exp chosen so that the largest |w - hi16| lands in [128, 256), and
    the fp32 row sums of hi16 + 2^-exp W8."""
    import math
    w = w.detach().float().contiguous()
    hi = convert_h16(w, prec)
    lo = (w - hi.float()).cpu()
    mx = float(lo.abs().max())
    e = 7 - int(math.floor(math.log2(mx))) if mx > 0 else 0
    e = max(-100, min(100, e))
    q = (lo * (2.0 ** e)).to(torch.float8_e4m3fn)          # OCP e4m3 (gfx950), round to nearest even, on the host
    N, K = w.shape
    w8 = torch.zeros(N, 4 * K, dtype=torch.uint8)
    w8[:, :K] = q.view(torch.uint8)
    s8 = (hi.float().cpu().double() + q.to(torch.float32).double() * (2.0 ** -e)).sum(1).float()
    return hi, w8.to(w.device), e, s8.to(w.device).contiguous()


def convert_h16(x, prec, out=None):
    """fp32 -> 16-bit copy in `prec`; into `out` (contiguous, same number of elements) when given."""
    x = x.contiguous()
    if out is None:
        out = torch.empty(x.shape, dtype=h16_dtype(prec), device=x.device)
    assert out.is_contiguous() and out.numel() == x.numel() and out.dtype == h16_dtype(prec)
    check(load().gava_convert_h16(ptr(x), ptr(out), x.numel(), prec, stream_ptr()), "gava_convert_h16")
    return out


def clip_lut(mean, std, device):
    """fp32 [3][256] with (v/255 - mean[c]) / std[c] for every byte value, evaluated with the reference's own torch expression
    (video_dataset/dataset.py:119,121) on the host: the GPU kernels look the normalised value up."""
    v = torch.arange(256, dtype=torch.float32).view(1, 256) / 255.
    lut = (v - torch.tensor(mean, dtype=torch.float32).view(3, 1)) / torch.tensor(std, dtype=torch.float32).view(3, 1)
    return lut.contiguous().to(device)


def preprocess_clip(frames_u8, out, *, T, rate, size, mean, std, first_temporal_view=False, first_spatial_view=False, lut=None):
    """frames_u8: uint8 [n][H][W][3] (device); out: fp32 view [3][T][size][size] whose last two dims are contiguous."""
    assert frames_u8.dtype == torch.uint8 and frames_u8.dim() == 4 and frames_u8.shape[-1] == 3 and frames_u8.is_contiguous()
    assert out.dtype == torch.float32 and tuple(out.shape) == (3, T, size, size)
    assert out.stride(3) == 1 and out.stride(2) == size, "output planes must be contiguous"
    a = PreprocessArgs()
    a.frames, a.n_frames, a.height, a.width = ptr(frames_u8), frames_u8.shape[0], frames_u8.shape[1], frames_u8.shape[2]
    a.mean, a.std = (C.c_float * 3)(*[float(v) for v in mean]), (C.c_float * 3)(*[float(v) for v in std])
    a.T, a.rate, a.size = T, rate, size
    a.out, a.out_stride_c, a.out_stride_t = ptr(out), out.stride(0), out.stride(1)
    a.first_temporal_view, a.first_spatial_view = int(first_temporal_view), int(first_spatial_view)
    a.lut = ptr(lut)
    check(load().gava_preprocess_clip(C.byref(a), stream_ptr()), "gava_preprocess_clip")


def preprocess_clips(desc, out, *, T, size, lut):
    """The whole batch in one launch: desc = device array of B gava_clip_desc (clip_descriptors / clip_descriptors_box),
    out = fp32 [B][3][T][size][size] whose size x size planes are contiguous, lut = clip_lut(...)."""
    B = out.shape[0]
    assert out.dtype == torch.float32 and tuple(out.shape) == (B, 3, T, size, size)
    assert out.stride(4) == 1 and out.stride(3) == size, "output planes must be contiguous"
    assert desc.dtype == torch.uint8 and desc.numel() == B * C.sizeof(ClipDesc) and lut is not None
    a = PreprocessClipsArgs()
    a.clips, a.lut, a.B, a.T, a.size = ptr(desc), ptr(lut), B, T, size
    a.out, a.out_stride_b, a.out_stride_c, a.out_stride_t = ptr(out), out.stride(0), out.stride(1), out.stride(2)
    check(load().gava_preprocess_clips(C.byref(a), stream_ptr()), "gava_preprocess_clips")


def patchify(out, *, B, T, size, patch, prec, x=None, clips=None, clip_lut=None):
    """16-bit patch matrix [B*T*(size/patch)^2, ldo] of the fp32 clips `x` (B,3,T,size,size) or of the uint8 videos behind
    `clips` (clip_descriptors): the A operand of the patch-embedding GEMM (gemm(A, ..., epilogue=EPI_F32_PATCH))."""
    a = PatchifyArgs()
    a.x, a.clips, a.clip_lut = ptr(x), ptr(clips), ptr(clip_lut)
    a.B, a.T, a.size, a.patch, a.prec = B, T, size, patch, prec
    a.out, a.ldo = ptr(out), out.stride(0)
    check(load().gava_patchify(C.byref(a), stream_ptr()), "gava_patchify")


def unpatchify(dpatch, out, *, B, T, size, patch, mode, frame_rows, row_offset, x=None):
    """The fold half of the patch embedding (gava_unpatchify, the inverse of patchify's index map): dpatch fp32
    [B*T*frame_rows, ld] (or [B*T, frame_rows, ld]), of which rows row_offset ... row_offset + (size/patch)^2 - 1 of every
    frame and columns [0, 3*patch^2) are read -> out fp32 [B, 3, T, size, size] (mode UNPATCH_GRAD) or the map [B, T, size,
    size] of UNPATCH_ABSMAX / UNPATCH_L2 / UNPATCH_GRAD_X_INPUT; the last one takes the fp32 clip x [B, 3, T, size, size]."""
    _require(mode in (UNPATCH_GRAD, UNPATCH_ABSMAX, UNPATCH_L2, UNPATCH_GRAD_X_INPUT), f"unpatchify: unknown mode {mode!r}")
    _require((mode == UNPATCH_GRAD_X_INPUT) == (x is not None), "unpatchify: x goes with mode UNPATCH_GRAD_X_INPUT and with no other")
    for name, t in (("dpatch", dpatch), ("out", out), ("x", x)):
        _require(t is None or (torch.is_tensor(t) and t.dtype == torch.float32 and t.is_contiguous()),
                 f"unpatchify: {name} must be a contiguous fp32 tensor")
    _require(min(B, T, size, patch) > 0 and size % patch == 0, f"unpatchify: B={B} T={T} size={size} patch={patch}")
    n = (size // patch) ** 2
    _require(dpatch.dim() in (2, 3) and dpatch.numel() == B * T * frame_rows * dpatch.shape[-1] and
             (dpatch.dim() == 2 or dpatch.shape[1] == frame_rows),
             f"unpatchify: dpatch {tuple(dpatch.shape)} is not {B * T} frames of {frame_rows} rows")
    _require(dpatch.shape[-1] >= 3 * patch * patch, f"unpatchify: rows of {dpatch.shape[-1]} floats hold no {3 * patch * patch} patch columns")
    _require(0 <= row_offset and row_offset + n <= frame_rows, f"unpatchify: rows {row_offset} ... {row_offset + n - 1} of a frame of {frame_rows}")
    clip = (B, 3, T, size, size)
    want = clip if mode == UNPATCH_GRAD else (B, T, size, size)
    _require(tuple(out.shape) == want, f"unpatchify: out is {tuple(out.shape)}, this mode writes {want}")
    _require(x is None or tuple(x.shape) == clip, f"unpatchify: x is {tuple(x.shape) if x is not None else None}, not {clip}")
    for name, t in (("dpatch", dpatch), ("out", out), ("x", x)):
        _require(t is None or t.is_cuda, f"unpatchify: {name} must be on the HIP device: there is no CPU fallback")
    _require(dpatch.device == out.device and (x is None or x.device == out.device), "unpatchify: tensors on different devices")
    a = UnpatchifyArgs()
    a.dpatch, a.ld, a.x, a.out = ptr(dpatch), dpatch.shape[-1], ptr(x), ptr(out)
    a.B, a.T, a.size, a.patch, a.mode, a.frame_rows, a.row_offset = B, T, size, patch, mode, frame_rows, row_offset
    with torch.cuda.device(out.device):
        check(load().gava_unpatchify(C.byref(a), stream_ptr(out.device)), "gava_unpatchify")
    return out


def attention_mass(q, k, out=None, *, batch, heads, n_q, n_kmain, prec, w=None, renorm=False,
                   side_k=None, n_g=0, T=0, has_summary=False, q_batch_rows=0):
    """Where the attention goes (gava_attention_mass): out[f, h, j] = sum_i w[f, i] * softmax_j(q_i . k_j), operands addressed
    as by `attention` (q pre-scaled h16, possibly a buffer of its own with q_batch_rows rows per frame; side_k = the prompt
    rows' keys).  renorm: P restricted to the frame's own n_kmain keys and renormalised per query.  w: fp32 [batch, n_q] or
    None (all ones).  -> out fp32 [batch, heads, n_kmain (renorm) or n_kmain + n_side], allocated when not given.  One
    launch, no sync; at most ATTENTION_MASS_MAX_KEYS keys."""
    for name, t in (("q", q), ("k", k), ("side_k", side_k), ("w", w), ("out", out)):
        _require(t is None or (torch.is_tensor(t) and t.is_cuda), f"attention_mass: {name} must be on the HIP device: there is no CPU fallback")
    n_side = (n_g + T + int(bool(has_summary))) if side_k is not None else 0
    n_out = n_kmain if renorm else n_kmain + n_side
    _require(n_kmain + n_side <= ATTENTION_MASS_MAX_KEYS,
             f"attention_mass: {n_kmain + n_side} keys, at most {ATTENTION_MASS_MAX_KEYS} are supported")
    _require(w is None or (w.dtype == torch.float32 and w.is_contiguous() and w.numel() == batch * n_q),
             "attention_mass: w must be a contiguous fp32 [batch, n_q] tensor")
    if out is None:
        out = torch.empty(batch, heads, n_out, dtype=torch.float32, device=q.device)
    _require(out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (batch, heads, n_out),
             f"attention_mass: out must be a contiguous fp32 {(batch, heads, n_out)} tensor")
    a = AttentionMassArgs()
    a.q, a.k, a.ld_qkv = ptr(q), ptr(k), k.stride(0)
    a.side_k, a.ld_side = ptr(side_k), (side_k.stride(0) if side_k is not None else 0)
    a.w, a.out = ptr(w), ptr(out)
    a.batch, a.heads, a.n_q, a.n_kmain = batch, heads, n_q, n_kmain
    a.n_g, a.T, a.has_summary = (n_g, T, int(bool(has_summary))) if side_k is not None else (0, 0, 0)
    a.renorm, a.prec = int(bool(renorm)), prec
    a.q_batch_rows, a.ld_q = q_batch_rows, (q.stride(0) if q_batch_rows else 0)
    with torch.cuda.device(out.device):
        check(load().gava_attention_mass(C.byref(a), stream_ptr(out.device)), "gava_attention_mass")
    return out


def attention_relevance(q, k, v, dout, out=None, *, batch, heads, n_q, n_kmain, prec, w=None, act_prec=None,
                        side_k=None, n_g=0, T=0, has_summary=False, q_batch_rows=0):
    """One step of gradient-weighted attention relevance (gava_attention_relevance): out[f, h, j] = sum_i w[f, i] *
    max(0, P[i, j] * G[i, j]) over the frame's own n_kmain keys, P = softmax_j(q_i . k_j) over ALL keys (side_k = the prompt
    rows' keys, not renormalised), G[i, j] = dout_i . v_j per head.  q / k / v / side_k are h16 of act_prec (None: of prec), q
    pre-scaled; dout is h16 of prec.  With q_batch_rows, q and dout are buffers of their own holding q_batch_rows rows per
    frame.  w: fp32 [batch, n_q] or None (all ones).  -> out fp32 [batch, heads, n_kmain], allocated when not given.  One
    launch, no sync; at most ATTENTION_RELEVANCE_MAX_KEYS keys."""
    for name, t in (("q", q), ("k", k), ("v", v), ("dout", dout), ("side_k", side_k), ("w", w), ("out", out)):
        _require(t is None or (torch.is_tensor(t) and t.is_cuda), f"attention_relevance: {name} must be on the HIP device: there is no CPU fallback")
    n_side = (n_g + T + int(bool(has_summary))) if side_k is not None else 0
    _require(n_kmain + n_side <= ATTENTION_RELEVANCE_MAX_KEYS,
             f"attention_relevance: {n_kmain + n_side} keys, at most {ATTENTION_RELEVANCE_MAX_KEYS} are supported")
    _require(0 < n_q <= n_kmain and (q_batch_rows == 0 or q_batch_rows >= n_q), f"attention_relevance: n_q={n_q} n_kmain={n_kmain} q_batch_rows={q_batch_rows}")
    act = prec if act_prec is None else act_prec
    _require(prec in PREC_TORCH and act in PREC_TORCH, f"attention_relevance: unknown prec {prec!r} / act_prec {act_prec!r}")
    for name, t in (("q", q), ("k", k), ("v", v), ("side_k", side_k)):
        _require(t is None or (t.dtype == PREC_TORCH[act] and t.dim() == 2 and t.stride(1) == 1), f"attention_relevance: {name} must be {PREC_TORCH[act]} rows")
    _require(dout.dtype == PREC_TORCH[prec] and dout.dim() == 2 and dout.stride(1) == 1, f"attention_relevance: dout must be {PREC_TORCH[prec]} rows")
    qrows = batch * (q_batch_rows or n_q)
    _require(q.shape[0] >= qrows and dout.shape[0] >= qrows and min(q.shape[1], dout.shape[1]) >= heads * 64,
             f"attention_relevance: q {tuple(q.shape)} / dout {tuple(dout.shape)} hold no {qrows} rows of {heads} heads")
    _require(k.shape[0] >= batch * n_kmain and v.shape[0] >= batch * n_kmain and k.stride(0) == v.stride(0) and min(k.shape[1], v.shape[1]) >= heads * 64
             and (q_batch_rows or q.stride(0) == k.stride(0)),
             f"attention_relevance: k {tuple(k.shape)} / v {tuple(v.shape)} are not {batch * n_kmain} rows of one row stride")
    _require(side_k is None or (T > 0 and batch % T == 0 and side_k.shape[0] >= n_g + 2 * batch and side_k.shape[1] >= heads * 64),
             "attention_relevance: side_k must hold n_g + 2 * batch rows, batch whole clips of T frames")
    _require(w is None or (w.dtype == torch.float32 and w.is_contiguous() and w.numel() == batch * n_q),
             "attention_relevance: w must be a contiguous fp32 [batch, n_q] tensor")
    if out is None:
        out = torch.empty(batch, heads, n_kmain, dtype=torch.float32, device=q.device)
    _require(out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (batch, heads, n_kmain),
             f"attention_relevance: out must be a contiguous fp32 {(batch, heads, n_kmain)} tensor")
    a = AttentionRelevanceArgs()
    a.q, a.k, a.v, a.ld_qkv = ptr(q), ptr(k), ptr(v), k.stride(0)
    a.side_k, a.ld_side = ptr(side_k), (side_k.stride(0) if side_k is not None else 0)
    a.dout, a.ld_dout, a.w, a.out = ptr(dout), dout.stride(0), ptr(w), ptr(out)
    a.batch, a.heads, a.n_q, a.n_kmain = batch, heads, n_q, n_kmain
    a.n_g, a.T, a.has_summary = (n_g, T, int(bool(has_summary))) if side_k is not None else (0, 0, 0)
    a.prec, a.act_prec_set, a.act_prec = prec, int(act_prec is not None), act
    a.q_batch_rows, a.ld_q = q_batch_rows, (q.stride(0) if q_batch_rows else 0)
    with torch.cuda.device(out.device):
        check(load().gava_attention_relevance(C.byref(a), stream_ptr(out.device)), "gava_attention_relevance")
    return out


# ---- faithfulness curves (gava_patch_ranks, gava_blur_clips, gava_perturb_clips, gava_perturb_scores) ---------------------------
# Every wrapper checks shapes and dtypes first and the device last, so that a wrong call is refused with the same words with or
# without a GPU; nothing reaches the library before all of it passed.

def _is_f32(t):
    return torch.is_tensor(t) and t.dtype == torch.float32 and t.is_contiguous()


def _on_device(what, *tensors):
    ts = [t for t in tensors if t is not None]
    _require(all(t.is_cuda for t in ts), f"{what}: every tensor must be on the HIP device: there is no CPU fallback")
    _require(all(t.device == ts[0].device for t in ts), f"{what}: tensors on different devices")


def perturb_thresholds(n, steps=10, fractions=None):
    """The abscissae of a perturbation curve and its thresholds: fractions (default linspace(0, 1, steps + 1); a given list must
    start at 0, end at 1 and increase strictly) -> (fractions as a list of floats, k) with k_s = floor(f_s * n + 0.5) in float64,
    n = units per ranking.  Host arithmetic only."""
    import math
    _require(isinstance(n, int) and n >= 1, f"perturb_thresholds: {n!r} units per ranking")
    if fractions is None:
        _require(isinstance(steps, int) and not isinstance(steps, bool) and steps >= 1, f"perturb_thresholds: steps must be an int >= 1, got {steps!r}")
        f = [s / steps for s in range(steps + 1)]
    else:
        try:
            f = [float(v) for v in (fractions.tolist() if torch.is_tensor(fractions) else fractions)]
        except (TypeError, ValueError):
            raise GavaError(f"perturb_thresholds: fractions must be a list of numbers, got {fractions!r}") from None
        _require(len(f) >= 2 and f[0] == 0.0 and f[-1] == 1.0, f"perturb_thresholds: fractions must start at 0 and end at 1, got {f}")
        _require(all(math.isfinite(v) for v in f) and all(b > a for a, b in zip(f, f[1:])),
                 f"perturb_thresholds: fractions must increase strictly, got {f}")
    _require(len(f) <= PERTURB_MAX_STEPS, f"perturb_thresholds: {len(f)} fractions, at most {PERTURB_MAX_STEPS} are supported")
    return f, [int(math.floor(v * n + 0.5)) for v in f]


def gaussian_taps(sigma):
    """The blur's taps: exp(-i^2 / 2 sigma^2) for |i| <= r = ceil(3 sigma), normalised in float64, then rounded to fp32 (host)."""
    import math
    _require(isinstance(sigma, (int, float)) and math.isfinite(sigma) and sigma > 0, f"gaussian_taps: sigma must be a positive number, got {sigma!r}")
    r = int(math.ceil(3.0 * sigma))
    _require(r <= BLUR_MAX_RADIUS, f"gaussian_taps: sigma {sigma} needs radius {r}, at most {BLUR_MAX_RADIUS} is supported")
    w = torch.exp(-torch.arange(-r, r + 1, dtype=torch.float64) ** 2 / (2.0 * float(sigma) ** 2))
    return (w / w.sum()).float()


def patch_ranks(scores, *, patch=None, scope="clip"):
    """Rank the units of a score map (gava_patch_ranks).  scores fp32: [B, T, g, g] (patch=None: the unit is a patch),
    [B, T, S, S] with patch=P (pixels, pooled to (S/P)^2 patches by the fp32 sum over each P x P patch) or [B, T] (the unit is a
    frame).  scope "clip": one ranking per clip; "frame": one per frame (patch units only).  -> int32 [B, T*g*g] or [B, T],
    rank 0 = the most important unit: descending by value, -0 == +0, ties to the lower index, NaNs after -inf.  At most
    PERTURB_MAX_UNITS units per ranking.  One launch (pixels: two, through a [B, T, g, g] workspace allocated here), no sync."""
    _require(scope in ("clip", "frame"), f"patch_ranks: scope must be 'clip' or 'frame', got {scope!r}")
    _require(_is_f32(scores) and scores.dim() in (2, 4), "patch_ranks: scores must be a contiguous fp32 [B, T, g, g], [B, T, S, S] or [B, T] tensor")
    _require(scores.numel() > 0, f"patch_ranks: scores {tuple(scores.shape)} hold nothing")
    B, T = scores.shape[:2]
    a = PatchRanksArgs()
    if scores.dim() == 2:
        _require(scope == "clip", "patch_ranks: scope='frame' ranks the patches of a frame; frame scores have one unit per frame")
        _require(patch is None, "patch_ranks: patch goes with the pixel layout [B, T, S, S]")
        a.layout, a.g, a.patch, n, total = RANK_FRAME, 1, 0, T, T
    else:
        S = scores.shape[2]
        _require(scores.shape[3] == S, f"patch_ranks: scores {tuple(scores.shape)} are not square maps")
        if patch is None:
            a.layout, a.g, a.patch = RANK_PATCH, S, 0
        else:
            _require(isinstance(patch, int) and patch >= 1 and S % patch == 0, f"patch_ranks: maps of {S} pixels are no whole patches of {patch!r}")
            a.layout, a.g, a.patch = RANK_PIXEL, S // patch, patch
        total = T * a.g * a.g
        n = total if scope == "clip" else a.g * a.g
    _require(n <= PERTURB_MAX_UNITS, f"patch_ranks: {n} units per ranking, at most {PERTURB_MAX_UNITS} are supported")
    _require(B * total < 2 ** 31, f"patch_ranks: {B * total} units in all")
    _on_device("patch_ranks", scores)
    ranks = torch.empty(B, total, dtype=torch.int32, device=scores.device)
    pooled = torch.empty(B, total, dtype=torch.float32, device=scores.device) if a.layout == RANK_PIXEL else None
    a.scores, a.ranks, a.pooled, a.B, a.T = ptr(scores), ptr(ranks), ptr(pooled), B, T
    a.scope = SCOPE_CLIP if scope == "clip" else SCOPE_FRAME
    with torch.cuda.device(scores.device):
        check(load().gava_patch_ranks(C.byref(a), stream_ptr(scores.device)), "gava_patch_ranks")
    return ranks


def blur_clips(x, taps, out=None):
    """Separable Gaussian blur of every (b, c, t) plane of the fp32 clips x [B, 3, T, S, S] with the fp32 taps [2r + 1]
    (gaussian_taps; r <= BLUR_MAX_RADIUS), the border replicated (gava_blur_clips).  -> out, shaped like x, allocated when not
    given; a workspace of x's size is allocated for the row pass.  Two launches, no sync."""
    _require(_is_f32(x) and x.dim() == 5 and x.shape[1] == 3 and x.shape[3] == x.shape[4] and x.numel() > 0,
             "blur_clips: x must be a contiguous fp32 [B, 3, T, S, S] tensor")
    _require(_is_f32(taps) and taps.dim() == 1 and taps.numel() % 2 == 1 and taps.numel() // 2 <= BLUR_MAX_RADIUS,
             f"blur_clips: taps must be a contiguous fp32 [2r + 1] tensor with r <= {BLUR_MAX_RADIUS}")
    _require(out is None or (_is_f32(out) and out.shape == x.shape and out.data_ptr() != x.data_ptr()),
             "blur_clips: out must be a contiguous fp32 tensor shaped like x, and not x itself")
    _require(x.is_cuda, "blur_clips: every tensor must be on the HIP device: there is no CPU fallback")
    taps = taps.to(x.device)
    _on_device("blur_clips", x, taps, out)
    if out is None:
        out = torch.empty_like(x)
    tmp = torch.empty_like(x)
    a = BlurClipsArgs()
    a.x, a.taps, a.tmp, a.out = ptr(x), ptr(taps), ptr(tmp), ptr(out)
    a.B, a.T, a.size, a.radius = x.shape[0], x.shape[2], x.shape[3], taps.numel() // 2
    with torch.cuda.device(x.device):
        check(load().gava_blur_clips(C.byref(a), stream_ptr(x.device)), "gava_blur_clips")
    return out


def perturb_clips(x, ranks, k, *, patch, mode, baseline=None, out=None):
    """The perturbed copies of the fp32 clips x [nb, 3, T, S, S] (gava_perturb_clips).  ranks int32 [nb, T*(S/patch)^2] (patch
    units, as patch_ranks writes them in either scope) or [nb, T] (frame units); k: a host list of S1 non-decreasing thresholds.
    mode "deletion": a pixel takes the baseline when its unit's rank < k_s, else x; "insertion": the reverse.  baseline: None
    (zero), fp32 [3] (one value per channel) or fp32 shaped like x.  -> out fp32 [nb, S1, 3, T, S, S], whose words are x's or
    the baseline's bit for bit; allocated when not given.  One launch, no sync."""
    _require(mode in ("deletion", "insertion"), f"perturb_clips: mode must be 'deletion' or 'insertion', got {mode!r}")
    _require(_is_f32(x) and x.dim() == 5 and x.shape[1] == 3 and x.shape[3] == x.shape[4] and x.numel() > 0,
             "perturb_clips: x must be a contiguous fp32 [nb, 3, T, S, S] tensor")
    nb, _, T, S, _ = x.shape
    _require(isinstance(patch, int) and patch >= 1 and S % patch == 0, f"perturb_clips: clips of {S} pixels are no whole patches of {patch!r}")
    g = S // patch
    _require(torch.is_tensor(ranks) and ranks.dtype == torch.int32 and ranks.is_contiguous() and ranks.dim() == 2 and ranks.shape[0] == nb
             and ranks.shape[1] in (T, T * g * g),
             f"perturb_clips: ranks must be a contiguous int32 [{nb}, {T * g * g}] (patch units) or [{nb}, {T}] (frame units) tensor")
    units = UNITS_PATCH if ranks.shape[1] == T * g * g else UNITS_FRAME        # (g = 1: the two are the same thing)
    try:
        k = [int(v) for v in k]
    except (TypeError, ValueError):
        raise GavaError(f"perturb_clips: k must be a list of ints, got {k!r}") from None
    _require(1 <= len(k) <= PERTURB_MAX_STEPS, f"perturb_clips: {len(k)} thresholds, between 1 and {PERTURB_MAX_STEPS} are supported")
    _require(k[0] >= 0 and all(b >= a for a, b in zip(k, k[1:])) and k[-1] < 2 ** 31, f"perturb_clips: thresholds must be non-negative and non-decreasing, got {k}")
    kind = BASELINE_ZERO
    if baseline is not None:
        _require(_is_f32(baseline) and (tuple(baseline.shape) == (3,) or baseline.shape == x.shape),
                 f"perturb_clips: baseline must be None, a contiguous fp32 [3] tensor or one shaped like x, got "
                 f"{(baseline.dtype, tuple(baseline.shape)) if torch.is_tensor(baseline) else type(baseline)}")
        kind = BASELINE_CHANNEL if baseline.dim() == 1 else BASELINE_TENSOR
    want = (nb, len(k), 3, T, S, S)
    _require(out is None or (_is_f32(out) and tuple(out.shape) == want), f"perturb_clips: out must be a contiguous fp32 {want} tensor")
    _on_device("perturb_clips", x, ranks, baseline, out)
    if x.data_ptr() % 16:
        x = x.clone()
    if kind == BASELINE_TENSOR and baseline.data_ptr() % 16:
        baseline = baseline.clone()
    if out is None:
        out = torch.empty(want, dtype=torch.float32, device=x.device)
    _require(out.data_ptr() % 16 == 0, "perturb_clips: out must be 16-byte aligned")
    a = PerturbClipsArgs()
    a.x, a.ranks, a.baseline, a.out = ptr(x), ptr(ranks), ptr(baseline), ptr(out)
    a.nb, a.T, a.size, a.patch, a.units = nb, T, S, patch, units
    a.mode = PERTURB_DELETION if mode == "deletion" else PERTURB_INSERTION
    a.baseline_kind, a.n_steps = kind, len(k)
    for s, v in enumerate(k):
        a.k[s] = v
    with torch.cuda.device(x.device):
        check(load().gava_perturb_clips(C.byref(a), stream_ptr(x.device)), "gava_perturb_clips")
    return out


def perturb_scores(logits, fractions, *, ref_step, target=None):
    """The curves of a perturbation run (gava_perturb_scores).  logits fp32 [nb * S1, C] (clip-major, then step; rows
    contiguous), fractions: a host list of S1 abscissae, target: int64 [nb] device tensor or None - then the top-1 class of
    each clip's row ref_step, found on the device.
    -> dict(logit fp32 [nb, S1] = the target's raw logit, prob fp32 [nb, S1] = its softmax probability, top1 int32 [nb, S1]
    (lowest class on ties), auc_logit / auc_prob fp32 [nb] = trapezoids over the fractions, target int64 [nb]).  A target
    outside [0, C) gives NaN for that clip's logit, prob and areas.  One launch, no sync."""
    try:
        f = [float(v) for v in fractions]
    except (TypeError, ValueError):
        raise GavaError(f"perturb_scores: fractions must be a list of numbers, got {fractions!r}") from None
    S1 = len(f)
    _require(1 <= S1 <= PERTURB_MAX_STEPS, f"perturb_scores: {S1} fractions, between 1 and {PERTURB_MAX_STEPS} are supported")
    _require(torch.is_tensor(logits) and logits.dtype == torch.float32 and logits.dim() == 2 and logits.shape[1] >= 1
             and (logits.shape[1] == 1 or logits.stride(1) == 1) and logits.stride(0) >= logits.shape[1],
             "perturb_scores: logits must be an fp32 [nb * S1, C] tensor with contiguous rows")
    _require(logits.shape[0] > 0 and logits.shape[0] % S1 == 0, f"perturb_scores: {logits.shape[0]} rows are no whole clips of {S1} steps")
    nb, Cn = logits.shape[0] // S1, logits.shape[1]
    _require(isinstance(ref_step, int) and 0 <= ref_step < S1, f"perturb_scores: ref_step {ref_step!r} is outside the {S1} steps")
    _require(target is None or (torch.is_tensor(target) and target.dtype == torch.int64 and tuple(target.shape) == (nb,) and target.is_contiguous()),
             f"perturb_scores: target must be None or a contiguous int64 [{nb}] tensor")
    _on_device("perturb_scores", logits, target)
    dev = logits.device
    res = dict(logit=torch.empty(nb, S1, dtype=torch.float32, device=dev), prob=torch.empty(nb, S1, dtype=torch.float32, device=dev),
               top1=torch.empty(nb, S1, dtype=torch.int32, device=dev), auc_logit=torch.empty(nb, dtype=torch.float32, device=dev),
               auc_prob=torch.empty(nb, dtype=torch.float32, device=dev), target=torch.empty(nb, dtype=torch.int64, device=dev))
    a = PerturbScoresArgs()
    a.logits, a.ld, a.target = ptr(logits), logits.stride(0), ptr(target)
    a.logit, a.prob, a.top1 = ptr(res["logit"]), ptr(res["prob"]), ptr(res["top1"])
    a.auc_logit, a.auc_prob, a.target_out = ptr(res["auc_logit"]), ptr(res["auc_prob"]), ptr(res["target"])
    a.nb, a.n_steps, a.C, a.ref_step = nb, S1, Cn, ref_step
    for s, v in enumerate(f):
        a.fractions[s] = v
    with torch.cuda.device(dev):
        check(load().gava_perturb_scores(C.byref(a), stream_ptr(dev)), "gava_perturb_scores")
    return res


# ---- path gradients: integrated gradients and SmoothGrad (gava_hip.h, "path gradients") -------------------------------------------

def path_rule(rule, steps):
    """The quadrature of integrated gradients on [0, 1] -> (alpha, w), two host lists of m floats (float64 arithmetic).
    "trapezoid": m = steps >= 2 points alpha_k = k / (m - 1), weights 1 / (m - 1) with the two end ones halved; the baseline and
    the clip itself are steps 0 and m - 1.  "gausslegendre": the steps >= 1 Gauss-Legendre nodes (numpy.polynomial.legendre.
    leggauss) mapped to [0, 1], between the two endpoints as zero-weight steps: m = steps + 2 (the endpoints cost two forwards
    and backwards of a clip and add nothing to the map; they are there for f(x0) and f(x)).  The weights sum to 1."""
    _require(rule in ("trapezoid", "gausslegendre"), f"path_rule: rule must be 'trapezoid' or 'gausslegendre', got {rule!r}")
    _require(isinstance(steps, int) and not isinstance(steps, bool), f"path_rule: steps must be an int, got {steps!r}")
    if rule == "trapezoid":
        _require(steps >= 2, f"path_rule: the trapezoid rule needs steps >= 2, got {steps}")
        m = steps
        alpha = [k / (m - 1) for k in range(m)]
        w = [(0.5 if k in (0, m - 1) else 1.0) / (m - 1) for k in range(m)]
    else:
        _require(steps >= 1, f"path_rule: the Gauss-Legendre rule needs steps >= 1, got {steps}")
        import numpy as np
        t, wt = np.polynomial.legendre.leggauss(steps)
        alpha = [0.0] + [float(0.5 * (v + 1.0)) for v in t] + [1.0]
        w = [0.0] + [float(0.5 * v) for v in wt] + [0.0]
        m = steps + 2
    _require(m <= PATH_MAX_STEPS, f"path_rule: {m} steps (endpoints included), at most {PATH_MAX_STEPS} are supported")
    return alpha, w


def _float_list(what, v, lo, hi):
    import math
    try:
        v = [float(s) for s in (v.tolist() if torch.is_tensor(v) else v)]
    except (TypeError, ValueError):
        raise GavaError(f"{what} must be a list of numbers, got {v!r}") from None
    _require(lo <= len(v) <= hi, f"{what}: {len(v)} values, between {lo} and {hi} are supported")
    _require(all(math.isfinite(s) for s in v), f"{what} must be finite, got {v}")
    return v


def _clip_baseline(what, x, baseline):
    """-> the baseline kind of None / fp32 [3] / fp32 shaped like x."""
    if baseline is None:
        return BASELINE_ZERO
    _require(_is_f32(baseline) and (tuple(baseline.shape) == (3,) or baseline.shape == x.shape),
             f"{what}: baseline must be None, a contiguous fp32 [3] tensor or one shaped like x, got "
             f"{(baseline.dtype, tuple(baseline.shape)) if torch.is_tensor(baseline) else type(baseline)}")
    return BASELINE_CHANNEL if baseline.dim() == 1 else BASELINE_TENSOR


def path_clips(x, *, patch, alpha=None, baseline=None, sigma=None, samples=None, seed=0, clip0=0, out=None):
    """The m near-copies of the fp32 clips x [nb, 3, T, S, S] (gava_path_clips) -> out fp32 [nb, m, 3, T, S, S], allocated when
    not given.  Either the straight line from a baseline - alpha: a host list of m values in [0, 1], out[b, k] = fma(alpha_k, x,
    (1 - alpha_k) x0), exactly x0 at 0 and x at 1; baseline: None (zero), fp32 [3] or fp32 shaped like x - or Gaussian noise -
    sigma: fp32 [nb] device tensor, samples = m, out[b, k] = fma(sigma_b, z, x) with z from Philox4x32-10 keyed by `seed` and
    counted by (element, k, clip0 + b): clip0 is the global index of x[0], so a batch cut into calls gets the same noise.
    One launch, no sync."""
    what = "path_clips"
    _require((alpha is None) != (sigma is None), f"{what}: give alpha (the line from a baseline) or sigma (noise), not both and not neither")
    _require(_is_f32(x) and x.dim() == 5 and x.shape[1] == 3 and x.shape[3] == x.shape[4] and x.numel() > 0,
             f"{what}: x must be a contiguous fp32 [nb, 3, T, S, S] tensor")
    nb, _, T, S, _ = x.shape
    _require(isinstance(patch, int) and patch >= 1 and S % patch == 0, f"{what}: clips of {S} pixels are no whole patches of {patch!r}")
    a = PathClipsArgs()
    if alpha is not None:
        _require(samples is None, f"{what}: samples goes with sigma")
        al = _float_list(f"{what}: alpha", alpha, 1, PATH_MAX_STEPS)
        _require(all(0.0 <= v <= 1.0 for v in al), f"{what}: alpha must lie in [0, 1], got {al}")
        kind, m, a.mode = _clip_baseline(what, x, baseline), len(al), PATH_LINE
        for k, v in enumerate(al):
            a.alpha[k], a.beta[k] = v, 1.0 - v           # (ctypes rounds the doubles to fp32)
    else:
        _require(baseline is None, f"{what}: a baseline goes with alpha")
        _require(isinstance(samples, int) and not isinstance(samples, bool) and 1 <= samples <= PATH_MAX_STEPS,
                 f"{what}: samples must be an int in [1, {PATH_MAX_STEPS}], got {samples!r}")
        _require(_is_f32(sigma) and tuple(sigma.shape) == (nb,), f"{what}: sigma must be a contiguous fp32 [{nb}] tensor")
        _require(S % 2 == 0, f"{what}: noise is drawn four floats at a time, an odd size {S} is not supported")
        _require(isinstance(seed, int) and 0 <= seed < 2 ** 64, f"{what}: seed must be an int in [0, 2^64), got {seed!r}")
        _require(isinstance(clip0, int) and 0 <= clip0 and clip0 + nb < 2 ** 31, f"{what}: clip0 {clip0!r} with {nb} clips")
        kind, m, a.mode, a.seed, a.clip0 = BASELINE_ZERO, samples, PATH_NOISE, seed, clip0
    want = (nb, m, 3, T, S, S)
    _require(out is None or (_is_f32(out) and tuple(out.shape) == want), f"{what}: out must be a contiguous fp32 {want} tensor")
    _on_device(what, x, baseline, sigma, out)
    if x.data_ptr() % 16:
        x = x.clone()
    if kind == BASELINE_TENSOR and baseline.data_ptr() % 16:
        baseline = baseline.clone()
    if out is None:
        out = torch.empty(want, dtype=torch.float32, device=x.device)
    _require(out.data_ptr() % 16 == 0, f"{what}: out must be 16-byte aligned")
    a.x, a.baseline, a.sigma, a.out = ptr(x), ptr(baseline), ptr(sigma), ptr(out)
    a.nb, a.T, a.size, a.patch, a.baseline_kind, a.m = nb, T, S, patch, kind, m
    with torch.cuda.device(x.device):
        check(load().gava_path_clips(C.byref(a), stream_ptr(x.device)), "gava_path_clips")
    return out


def clip_range(x, rel=1.0):
    """Per-clip range of the fp32 clips x [nb, 3, T, S, S] (gava_clip_range) -> (min, max, sigma), fp32 [nb] each, sigma =
    fl(rel * fl(max - min)): SmoothGrad's noise level relative to the clip's range.  Exact; a NaN in a clip makes its three
    values NaN.  Two launches through a small workspace allocated here, no sync."""
    import math
    _require(_is_f32(x) and x.dim() == 5 and x.shape[1] == 3 and x.shape[3] == x.shape[4] and x.numel() > 0,
             "clip_range: x must be a contiguous fp32 [nb, 3, T, S, S] tensor")
    _require(isinstance(rel, (int, float)) and not isinstance(rel, bool) and math.isfinite(rel), f"clip_range: rel must be a finite number, got {rel!r}")
    nb = x.shape[0]
    _require(nb <= 65535, f"clip_range: {nb} clips, at most 65535 go in one call")
    _on_device("clip_range", x)
    mn, mx, sg = (torch.empty(nb, dtype=torch.float32, device=x.device) for _ in range(3))
    ws = torch.empty(nb, CLIP_RANGE_PARTS, 2, dtype=torch.float32, device=x.device)
    a = ClipRangeArgs()
    a.x, a.min, a.max, a.sigma, a.workspace = ptr(x), ptr(mn), ptr(mx), ptr(sg), ptr(ws)
    a.nb, a.T, a.size, a.rel = nb, x.shape[2], x.shape[3], float(rel)
    with torch.cuda.device(x.device):
        check(load().gava_clip_range(C.byref(a), stream_ptr(x.device)), "gava_clip_range")
    return mn, mx, sg


def unpatchify_path(dpatch, out, *, B, T, size, patch, mode, frame_rows, row_offset, w, x=None, baseline=None):
    """unpatchify with the weighted sum over the m = len(w) copies of every clip folded in (gava_unpatchify_path): dpatch fp32
    holds the B*m*T frames of the copies (clip b's copy k is batch index b*m + k), out has B clips.  G_c = sum_k w_k g_c(b*m + k)
    as a chain of fused multiply-adds in k order, zero weights skipped; w: a host list.  mode PATH_GRAD -> out [B, 3, T, size,
    size] = G, PATH_ABSMAX / PATH_L2 -> [B, T, size, size], unpatchify's map rules on G; PATH_ATTR -> [B, 3, T, size, size] =
    (x - x0) * G, PATH_ATTR_SUM / PATH_ATTR_ABS -> [B, T, size, size], its channel sum / sum of magnitudes.  x (the fp32 clips
    [B, 3, T, size, size]) and baseline (None = zero, fp32 [3] or shaped like x) belong to the ATTR modes only."""
    what = "unpatchify_path"
    _require(mode in (PATH_GRAD, PATH_ABSMAX, PATH_L2, PATH_ATTR, PATH_ATTR_SUM, PATH_ATTR_ABS), f"{what}: unknown mode {mode!r}")
    attr = mode >= PATH_ATTR
    _require(attr == (x is not None), f"{what}: x goes with the PATH_ATTR modes and with no other")
    _require(attr or baseline is None, f"{what}: a baseline goes with the PATH_ATTR modes and with no other")
    for name, t in (("dpatch", dpatch), ("out", out), ("x", x)):
        _require(t is None or _is_f32(t), f"{what}: {name} must be a contiguous fp32 tensor")
    wl = _float_list(f"{what}: w", w, 1, PATH_MAX_STEPS)
    m = len(wl)
    _require(min(B, T, size, patch) > 0 and size % patch == 0, f"{what}: B={B} T={T} size={size} patch={patch}")
    n = (size // patch) ** 2
    _require(dpatch.dim() in (2, 3) and dpatch.numel() == B * m * T * frame_rows * dpatch.shape[-1] and
             (dpatch.dim() == 2 or dpatch.shape[1] == frame_rows),
             f"{what}: dpatch {tuple(dpatch.shape)} is not {B} x {m} x {T} frames of {frame_rows} rows")
    _require(dpatch.shape[-1] >= 3 * patch * patch, f"{what}: rows of {dpatch.shape[-1]} floats hold no {3 * patch * patch} patch columns")
    _require(0 <= row_offset and row_offset + n <= frame_rows, f"{what}: rows {row_offset} ... {row_offset + n - 1} of a frame of {frame_rows}")
    clip = (B, 3, T, size, size)
    want = clip if mode in (PATH_GRAD, PATH_ATTR) else (B, T, size, size)
    _require(tuple(out.shape) == want, f"{what}: out is {tuple(out.shape)}, this mode writes {want}")
    _require(x is None or tuple(x.shape) == clip, f"{what}: x is {tuple(x.shape) if x is not None else None}, not {clip}")
    kind = _clip_baseline(what, x, baseline) if attr else BASELINE_ZERO
    _on_device(what, dpatch, out, x, baseline)
    a = UnpatchifyPathArgs()
    a.dpatch, a.ld, a.x, a.baseline, a.out = ptr(dpatch), dpatch.shape[-1], ptr(x), ptr(baseline), ptr(out)
    a.B, a.T, a.size, a.patch, a.mode, a.baseline_kind = B, T, size, patch, mode, kind
    a.frame_rows, a.row_offset, a.m = frame_rows, row_offset, m
    for k, v in enumerate(wl):
        a.w[k] = v
    with torch.cuda.device(out.device):
        check(load().gava_unpatchify_path(C.byref(a), stream_ptr(out.device)), "gava_unpatchify_path")
    return out


def path_delta(attr, logits, target, *, m, k_lo, k_hi):
    """The completeness residual of integrated gradients (gava_path_delta).  attr: the signed map fp32 [B, T, S, S]; logits fp32
    [B * m, C] (row b*m + k, rows contiguous); target int64 [B] device tensor; k_lo / k_hi: the steps that are the baseline and
    the clip.  -> dict(sum_attr, f_diff, delta), fp32 [B] each: the clip's summed attribution (added in double in a fixed order,
    rounded once), logits[b*m + k_hi, target] - logits[b*m + k_lo, target], and their difference.  A target outside [0, C)
    gives NaN for that clip.  One launch, no sync."""
    what = "path_delta"
    _require(_is_f32(attr) and attr.dim() == 4 and attr.shape[2] == attr.shape[3] and attr.numel() > 0,
             f"{what}: attr must be a contiguous fp32 [B, T, S, S] tensor")
    B = attr.shape[0]
    _require(isinstance(m, int) and not isinstance(m, bool) and 1 <= m <= PATH_MAX_STEPS, f"{what}: m must be an int in [1, {PATH_MAX_STEPS}], got {m!r}")
    _require(torch.is_tensor(logits) and logits.dtype == torch.float32 and logits.dim() == 2 and logits.shape[1] >= 1
             and (logits.shape[1] == 1 or logits.stride(1) == 1) and logits.stride(0) >= logits.shape[1],
             f"{what}: logits must be an fp32 [B * m, C] tensor with contiguous rows")
    _require(logits.shape[0] == B * m, f"{what}: {logits.shape[0]} rows of logits are not {B} clips of {m} steps")
    for name, k in (("k_lo", k_lo), ("k_hi", k_hi)):
        _require(isinstance(k, int) and 0 <= k < m, f"{what}: {name} {k!r} is outside the {m} steps")
    _require(torch.is_tensor(target) and target.dtype == torch.int64 and tuple(target.shape) == (B,) and target.is_contiguous(),
             f"{what}: target must be a contiguous int64 [{B}] tensor")
    _on_device(what, attr, logits, target)
    dev = attr.device
    res = {k: torch.empty(B, dtype=torch.float32, device=dev) for k in ("sum_attr", "f_diff", "delta")}
    a = PathDeltaArgs()
    a.map, a.logits, a.ld, a.target = ptr(attr), ptr(logits), logits.stride(0), ptr(target)
    a.sum_attr, a.f_diff, a.delta = ptr(res["sum_attr"]), ptr(res["f_diff"]), ptr(res["delta"])
    a.B, a.T, a.size, a.m, a.C, a.k_lo, a.k_hi = B, attr.shape[1], attr.shape[2], m, logits.shape[1], k_lo, k_hi
    with torch.cuda.device(dev):
        check(load().gava_path_delta(C.byref(a), stream_ptr(dev)), "gava_path_delta")
    return res


# ---- backward ops ------------------------------------------------------------

def layernorm_backward(x, gamma, dy, dx, *, accumulate=False, x_row_index=None, dx_row_index=None, rows=None,
                       dgamma=None, dbeta=None, dx16=None, prec=PREC_BF16):
    a = LayerNormBwdArgs()
    a.dx16, a.dx16_stride, a.prec = ptr(dx16), (dx16.stride(0) if dx16 is not None else 0), prec
    a.x, a.x_stride, a.x_row_index = ptr(x), x.stride(0), ptr(x_row_index)
    a.gamma, a.dy, a.dy_stride = ptr(gamma), ptr(dy), dy.stride(0)
    a.dx, a.dx_stride, a.dx_row_index = ptr(dx), dx.stride(0), ptr(dx_row_index)
    a.dgamma, a.dbeta = ptr(dgamma), ptr(dbeta)
    a.rows, a.D, a.accumulate = (dy.shape[0] if rows is None else rows), x.shape[-1], int(accumulate)
    check(load().gava_layernorm_backward(C.byref(a), stream_ptr()), "gava_layernorm_backward")


def qgelu_backward(pre, dh, dpre, prec):
    assert pre.is_contiguous() and dh.is_contiguous() and dpre.is_contiguous() and pre.numel() == dh.numel() == dpre.numel()
    check(load().gava_qgelu_backward(ptr(pre), ptr(dh), ptr(dpre), pre.numel(), prec, stream_ptr()), "gava_qgelu_backward")


def attention_backward(q, k, v, dout, dq, dk, dv, *, batch, heads, n, prec, causal=False, q_scale=1.0,
                       side_k=None, side_v=None, dside_k=None, dside_v=None, n_g=0, T=0, has_summary=False, n_q=0,
                       act_prec=None, q_batch_rows=0):
    a = AttentionBwdArgs()
    a.q_batch_rows, a.ld_q, a.ld_dq = q_batch_rows, (q.stride(0) if q_batch_rows else 0), (dq.stride(0) if q_batch_rows else 0)
    a.act_prec_set, a.act_prec = int(act_prec is not None), (act_prec if act_prec is not None else prec)
    a.side_k, a.side_v = ptr(side_k), ptr(side_v)
    a.ld_side = side_k.stride(0) if side_k is not None else 0
    a.dside_k, a.dside_v = ptr(dside_k), ptr(dside_v)
    a.ld_dside = dside_k.stride(0) if dside_k is not None else 0
    a.n_g, a.T, a.has_summary, a.n_q = n_g, T, int(has_summary), n_q
    ws = torch.empty(load().gava_attention_backward_workspace_bytes(batch, heads, n_q or n), dtype=torch.uint8, device=q.device)
    a.workspace = ptr(ws)
    a.q, a.k, a.v, a.ld_qkv = ptr(q), ptr(k), ptr(v), k.stride(0)
    a.dout, a.ld_dout = ptr(dout), dout.stride(0)
    a.dq, a.dk, a.dv, a.ld_dqkv = ptr(dq), ptr(dk), ptr(dv), dk.stride(0)
    a.batch, a.heads, a.n, a.causal, a.prec, a.q_scale = batch, heads, n, int(causal), prec, q_scale
    check(load().gava_attention_backward(C.byref(a), stream_ptr()), "gava_attention_backward")


def row_stats(rowsum, D):
    """float2 partial sums [rows][slots] of the folding producers -> (mean, rstd) float2 [rows]."""
    rows, slots = rowsum.shape[0], rowsum.shape[1]
    stats = torch.empty(rows, 2, dtype=torch.float32, device=rowsum.device)
    check(load().gava_row_stats(ptr(rowsum), slots, D, rows, ptr(stats), stream_ptr()), "gava_row_stats")
    return stats


def clip_descriptors(videos, *, T, rate, size, first_temporal_view=False, first_spatial_view=False):
    """uint8 videos [n_i][H_i][W_i][3] on the device -> (uint8 device tensor holding an array of gava_clip_desc, keep-alive
    list).  The geometry is computed by the library (gava_clip_geometry: dataset.py:124-129,163-186)."""
    lib = load()
    arr = (ClipDesc * len(videos))()
    for i, v in enumerate(videos):
        assert v.is_cuda and v.dtype == torch.uint8 and v.dim() == 4 and v.shape[-1] == 3 and v.is_contiguous()
        arr[i].frames, arr[i].n_frames, arr[i].height, arr[i].width = ptr(v), v.shape[0], v.shape[1], v.shape[2]
        check(lib.gava_clip_geometry(C.byref(arr[i]), T, rate, size, int(first_temporal_view), int(first_spatial_view)),
              "gava_clip_geometry")
    host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
    return host.to(videos[0].device), list(videos)


def clip_descriptors_box(videos, draws, *, size):
    """The random-sample branch (dataset.py:93-114, auto_augment=None): `draws` holds one (idx, i, j, h, w) per video -
    source frame indices and the crop box of transform.py:503-542 - checked by the library (gava_clip_geometry_box).
    -> (uint8 device tensor holding an array of gava_clip_desc, keep-alive list: the videos and the device frame tables)."""
    lib = load()
    arr = (ClipDesc * len(videos))()
    T = len(draws[0][0])
    assert all(len(d[0]) == T for d in draws) and len(draws) == len(videos)
    dev = videos[0].device
    tables = torch.tensor([list(d[0]) for d in draws], dtype=torch.int32).to(dev)       # one copy for the batch
    for n, (v, (idx, i, j, h, w)) in enumerate(zip(videos, draws)):
        assert v.is_cuda and v.dtype == torch.uint8 and v.dim() == 4 and v.shape[-1] == 3 and v.is_contiguous()
        arr[n].frames, arr[n].n_frames, arr[n].height, arr[n].width = ptr(v), v.shape[0], v.shape[1], v.shape[2]
        host = (C.c_int * T)(*[int(x) for x in idx])
        check(lib.gava_clip_geometry_box(C.byref(arr[n]), size, T, host, ptr(tables[n]), int(i), int(j), int(h), int(w)),
              "gava_clip_geometry_box")
    host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
    return host.to(dev), list(videos) + [tables]


def clip_descriptors_views(videos, *, T, rate, size, n_spatial, n_temporal):
    """Every evaluation crop of every video (dataset.py:135-136 builds n_spatial x n_temporal of them): -> (uint8 device tensor
    holding B*V gava_clip_desc, video-major with a video's V views in upstream's order view = sv * n_temporal + tv; keep-alive
    list; host int32 array [B*V, 3] with each clip's (t_st, h_st, w_st)).  Geometry by the library (gava_clip_geometry_view)."""
    import numpy as np
    lib = load()
    V = n_spatial * n_temporal
    arr = (ClipDesc * (len(videos) * V))()
    for b, v in enumerate(videos):
        assert v.is_cuda and v.dtype == torch.uint8 and v.dim() == 4 and v.shape[-1] == 3 and v.is_contiguous()
        for k in range(V):
            d = arr[b * V + k]
            d.frames, d.n_frames, d.height, d.width = ptr(v), v.shape[0], v.shape[1], v.shape[2]
            check(lib.gava_clip_geometry_view(C.byref(d), T, rate, size, n_spatial, n_temporal, k), "gava_clip_geometry_view")
    raw = np.frombuffer(bytes(arr), dtype=np.uint8).reshape(len(arr), C.sizeof(ClipDesc))
    first = ClipDesc.t_st.offset
    assert ClipDesc.h_st.offset == first + 8 and ClipDesc.w_st.offset == first + 12
    geom = raw[:, first:first + 16].copy().view(np.int32)[:, [0, 2, 3]]
    return torch.from_numpy(raw.copy()).reshape(-1).to(videos[0].device), list(videos), geom


def view_scores(logits):
    """Multi-view score fusion (gava_view_scores): logits = fp32 device tensor [B, V, C] whose last dimension is contiguous (any
    video / view strides) -> (scores fp32 [B, C] = mean over the views of softmax over the classes, top1 int32 [B] = its argmax,
    the lowest class on ties).  One launch, no sync."""
    assert logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 3, "logits must be a device fp32 [B, V, C] tensor"
    B, V, Cn = logits.shape
    assert Cn == 1 or logits.stride(2) == 1, "the class dimension must be contiguous"
    scores = torch.empty(B, Cn, dtype=torch.float32, device=logits.device)
    top1 = torch.empty(B, dtype=torch.int32, device=logits.device)
    a = ViewScoresArgs()
    a.logits, a.ld_video, a.ld_view = ptr(logits), logits.stride(0), logits.stride(1)
    a.B, a.V, a.C, a.scores, a.top1 = B, V, Cn, ptr(scores), ptr(top1)
    with torch.cuda.device(logits.device):
        check(load().gava_view_scores(C.byref(a), stream_ptr(logits.device)), "gava_view_scores")
    return scores, top1


# ---- training head and criterion (gava_train_criterion*, gava_train_head*) ----------------------------------------------------

def _f32(t, what):
    assert t.is_cuda and t.dtype == torch.float32, f"{what} must be a device fp32 tensor"
    return t


def train_criterion(logits, labels, *, weighted=False, alpha=0.25, gamma=2.0, beta=0.0, scale=1.0, conf=None, check_labels=False):
    """Per-sample cross-entropy (times the ordinal-focal weight when `weighted`), its mean, the argmax and the hit count
    (gava_train_criterion; the formula is in include/gava_hip.h).  logits: device fp32 [B, C] with a contiguous class dimension
    (any row stride); labels: device int64 [B].  conf: optional device int32 [C, C], ACCUMULATED: conf[label, top1] += 1.
    -> dict(loss (0-dim), per_sample [B], weight [B], top1 int32 [B], hits int32 (0-dim), conf, saved [B, 4]).
    Labels outside [0, C) are clamped by the kernel; check_labels=True refuses them here instead, at the price of a host
    sync.  Two launches, no sync otherwise."""
    _f32(logits, "logits")
    assert logits.dim() == 2 and (logits.shape[1] == 1 or logits.stride(1) == 1), "logits must be [B, C] with a contiguous class dimension"
    if labels.is_floating_point() or labels.dim() != 1:
        raise GavaError("gava_train_criterion takes integer class labels [B]; soft (mixup) targets are not supported")
    B, Cn = logits.shape
    assert labels.shape[0] == B and labels.is_cuda
    labels = labels.to(torch.int64).contiguous()
    if check_labels and bool(((labels < 0) | (labels >= Cn)).any()):
        raise GavaError(f"labels outside [0, {Cn})")
    dev = logits.device
    out = dict(loss=torch.empty((), dtype=torch.float32, device=dev), per_sample=torch.empty(B, dtype=torch.float32, device=dev),
               weight=torch.empty(B, dtype=torch.float32, device=dev), top1=torch.empty(B, dtype=torch.int32, device=dev),
               hits=torch.empty((), dtype=torch.int32, device=dev), conf=conf,
               saved=torch.empty(B, 4, dtype=torch.float32, device=dev))
    if conf is not None:
        assert conf.is_cuda and conf.dtype == torch.int32 and tuple(conf.shape) == (Cn, Cn) and conf.is_contiguous()
    a = TrainCriterionArgs()
    a.logits, a.ld_logits, a.labels = ptr(logits), (logits.stride(0) if B > 1 else max(logits.stride(0), Cn)), ptr(labels)
    a.B, a.C, a.weighted = B, Cn, int(weighted)
    a.alpha, a.gamma, a.beta, a.scale = alpha, gamma, beta, scale
    a.loss, a.per_sample, a.weight, a.top1, a.hits = ptr(out["loss"]), ptr(out["per_sample"]), ptr(out["weight"]), ptr(out["top1"]), ptr(out["hits"])
    a.conf, a.saved = ptr(conf), ptr(out["saved"])
    with torch.cuda.device(dev):
        check(load().gava_train_criterion(C.byref(a), stream_ptr(dev)), "gava_train_criterion")
    out["labels"] = labels
    return out


def train_criterion_backward(logits, labels, saved, grad_loss):
    """dlogits [B, C] of train_criterion's loss; grad_loss: the upstream gradient, a DEVICE fp32 scalar (never read on the host)."""
    _f32(logits, "logits"), _f32(grad_loss, "grad_loss")
    B, Cn = logits.shape
    assert grad_loss.numel() == 1 and labels.dtype == torch.int64 and labels.is_contiguous() and tuple(saved.shape) == (B, 4)
    dlogits = torch.empty(B, Cn, dtype=torch.float32, device=logits.device)
    a = TrainCriterionArgs()
    a.logits, a.ld_logits, a.labels = ptr(logits), (logits.stride(0) if B > 1 else max(logits.stride(0), Cn)), ptr(labels)
    a.B, a.C, a.saved, a.grad_loss, a.dlogits, a.ld_dlogits = B, Cn, ptr(saved), ptr(grad_loss), ptr(dlogits), Cn
    with torch.cuda.device(logits.device):
        check(load().gava_train_criterion_backward(C.byref(a), stream_ptr(logits.device)), "gava_train_criterion_backward")
    return dlogits


# ---- Mixup / CutMix and the criterion for soft targets (gava_mix_*, gava_soft_criterion*) ---------------------------------------

def mix_descriptors(plan, H, W, device=None):
    """The host plan of a mix - dict(partner int [B], lam float [B], box int [B, 4] as (y0, y1, x0, x1)) - as the ABI's
    descriptor table, twice: -> dict(host = pinned uint8 tensor holding B gava_mix_desc (what gava_mix_clips validates),
    dev = its device copy (what the kernels read), B, H, W).  The copy is non-blocking from pinned memory on the current
    stream; nothing waits for it."""
    import numpy as np
    partner = np.ascontiguousarray(plan["partner"], dtype=np.int32).reshape(-1)
    B = partner.shape[0]
    lam = np.ascontiguousarray(plan["lam"], dtype=np.float32).reshape(-1)
    box = np.ascontiguousarray(plan["box"], dtype=np.int32).reshape(-1, 4)
    _require(lam.shape[0] == B and box.shape[0] == B and B >= 1, "mix_descriptors: partner [B], lam [B] and box [B, 4] must agree")
    host = torch.empty(B * C.sizeof(MixDesc), dtype=torch.uint8).pin_memory()
    rows = host.numpy().view(np.int32).reshape(B, 6)
    rows[:, 0], rows[:, 1], rows[:, 2:] = partner, lam.view(np.int32), box
    dev = host.to(device if device is not None else torch.device("cuda", torch.cuda.current_device()), non_blocking=True)
    return dict(host=host, dev=dev, B=B, H=int(H), W=int(W))


def mix_clips(x, desc, out=None):
    """Mixup / CutMix of a batch of clips by `desc` (mix_descriptors): gava_mix_clips.  x: contiguous device fp32
    [B, ..., H, W]; out: None (a new tensor), x itself (in place; the partners must then pair up) or another contiguous
    tensor of x's shape.  -> out.  The descriptors are validated by the library before any launch."""
    _on_device("mix_clips", x)
    _require(_is_f32(x) and x.dim() >= 3 and x.is_contiguous(), "mix_clips: x must be a contiguous fp32 [B, ..., H, W] tensor")
    B, H, W = x.shape[0], x.shape[-2], x.shape[-1]
    _require(B >= 1 and x.numel() > 0, "mix_clips: x is empty")
    _require((desc["B"], desc["H"], desc["W"]) == (B, H, W), "mix_clips: the descriptors were made for another batch or image size")
    _require(desc["dev"].device == x.device, "mix_clips: the descriptor table is on another device")
    if out is None:
        out = torch.empty_like(x)
    _require(out.is_cuda and out.device == x.device and _is_f32(out) and out.shape == x.shape and out.is_contiguous(),
             "mix_clips: out must be a contiguous fp32 tensor of x's shape on its device")
    a = MixClipsArgs()
    a.x, a.out, a.desc_host, a.desc = ptr(x), ptr(out), desc["host"].data_ptr(), ptr(desc["dev"])
    a.B, a.planes, a.H, a.W = B, x.numel() // (B * H * W), H, W
    with torch.cuda.device(x.device):
        check(load().gava_mix_clips(C.byref(a), stream_ptr(x.device)), "gava_mix_clips")
    return out


def mix_targets(labels, desc, C_, smoothing=0.0):
    """targets fp32 [B, C] = lam * s(label) + (1 - lam) * s(partner's label), s = the label smoothed by `smoothing`
    (gava_mix_targets).  labels: device integer [B] (clamped to [0, C) on the device).  One launch, no sync."""
    _on_device("mix_targets", labels)
    _require(not labels.is_floating_point() and labels.dim() == 1 and labels.shape[0] == desc["B"],
             "mix_targets takes integer class labels [B], one per descriptor")
    _require(0.0 <= float(smoothing) <= 1.0 and int(C_) >= 1, "mix_targets: smoothing must lie in [0, 1] and C >= 1")
    labels = labels.to(torch.int64).contiguous()
    targets = torch.empty(desc["B"], int(C_), dtype=torch.float32, device=labels.device)
    a = MixTargetsArgs()
    a.labels, a.desc, a.targets, a.ld_targets = ptr(labels), ptr(desc["dev"]), ptr(targets), int(C_)
    a.B, a.C, a.smoothing = desc["B"], int(C_), float(smoothing)
    with torch.cuda.device(labels.device):
        check(load().gava_mix_targets(C.byref(a), stream_ptr(labels.device)), "gava_mix_targets")
    return targets


# ---- RandAugment layers (gava_augment_*) ------------------------------------------------------------------------------------------

def augment_desc_dtype():
    """numpy's view of gava_augment_desc (a structured dtype with the struct's offsets)"""
    import numpy as np
    return np.dtype(AugmentDesc)


def augment_layer(rows, hist, luts, device, stages=("hist", "luts", "apply")):
    """One layer of an augmentation policy: `rows` is a numpy array of gava_augment_desc (augment_desc_dtype), one per frame;
    hist / luts the device buffers its slots index (int32 [n_hist, 4, 256], zero before the first layer; uint8 [n_luts, 3, 256];
    None where no row needs them).  The table goes to the device from pinned memory, non-blocking, and the three entry points
    run in order (`stages`: a subset, for measurements).  The library validates the host table before every launch.  Nothing
    waits.  -> (pinned host table, device table): keep them until the layer's successor is enqueued."""
    import numpy as np
    rows = np.ascontiguousarray(rows, dtype=augment_desc_dtype())
    _require(rows.ndim == 1 and rows.shape[0] >= 1, "augment_layer: rows must hold at least one gava_augment_desc")
    host = torch.empty(rows.nbytes, dtype=torch.uint8).pin_memory()
    host.numpy()[:] = rows.view(np.uint8)
    dev = host.to(device, non_blocking=True)
    a = AugmentArgs()
    a.desc_host, a.desc, a.n = host.data_ptr(), ptr(dev), rows.shape[0]
    if hist is not None:
        _require(hist.is_cuda and hist.dtype == torch.int32 and hist.is_contiguous() and hist.shape[1:] == (4, 256),
                 "augment_layer: hist must be a contiguous device int32 tensor [n, 4, 256]")
        a.hist, a.n_hist = ptr(hist), hist.shape[0]
    if luts is not None:
        _require(luts.is_cuda and luts.dtype == torch.uint8 and luts.is_contiguous() and luts.shape[1:] == (3, 256),
                 "augment_layer: luts must be a contiguous device uint8 tensor [n, 3, 256]")
        a.luts, a.n_luts = ptr(luts), luts.shape[0]
    lib = load()
    with torch.cuda.device(device):
        for stage in stages:
            check(getattr(lib, "gava_augment_" + stage)(C.byref(a), stream_ptr(device)), "gava_augment_" + stage)
    return host, dev


def _row_stride(t):
    return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])


def _soft_args(logits, targets, weighted, alpha, gamma, beta, scale):
    _f32(logits, "logits"), _f32(targets, "targets")
    assert logits.dim() == 2 and (logits.shape[1] == 1 or logits.stride(1) == 1), "logits must be [B, C] with a contiguous class dimension"
    assert targets.shape == logits.shape and (targets.shape[1] == 1 or targets.stride(1) == 1) and targets.device == logits.device, \
        "targets must be [B, C] like the logits, with a contiguous class dimension"
    a = SoftCriterionArgs()
    a.logits, a.ld_logits, a.targets, a.ld_targets = ptr(logits), _row_stride(logits), ptr(targets), _row_stride(targets)
    a.B, a.C, a.weighted = logits.shape[0], logits.shape[1], int(weighted)
    a.alpha, a.gamma, a.beta, a.scale = alpha, gamma, beta, scale
    return a


def soft_criterion(logits, targets, *, weighted=False, alpha=0.25, gamma=2.0, beta=0.0, scale=1.0, conf=None):
    """The criterion for targets of the logits' shape (gava_soft_criterion; the formula is in include/gava_hip.h): per-sample
    cross-entropy with class probabilities (times the ordinal-focal weight when `weighted`), its mean, both argmaxes and the
    hit count.  logits, targets: device fp32 [B, C] with a contiguous class dimension (any row stride).  conf: optional device
    int32 [C, C], ACCUMULATED: conf[target1, top1] += 1.
    -> dict(loss (0-dim), per_sample [B], weight [B], top1 int32 [B], target1 int32 [B], hits int32 (0-dim), conf, saved [B, 8]).
    Two launches, no sync."""
    if not torch.is_tensor(targets) or not targets.is_floating_point() or targets.dim() != 2:
        raise GavaError("gava_soft_criterion takes fp32 targets [B, C] of the logits' shape; integer class labels go to "
                        "train_criterion (TrainCriterion)")
    a = _soft_args(logits, targets, weighted, alpha, gamma, beta, scale)
    B, Cn, dev = a.B, a.C, logits.device
    out = dict(loss=torch.empty((), dtype=torch.float32, device=dev), per_sample=torch.empty(B, dtype=torch.float32, device=dev),
               weight=torch.empty(B, dtype=torch.float32, device=dev), top1=torch.empty(B, dtype=torch.int32, device=dev),
               target1=torch.empty(B, dtype=torch.int32, device=dev), hits=torch.empty((), dtype=torch.int32, device=dev), conf=conf,
               saved=torch.empty(B, 8, dtype=torch.float32, device=dev))
    if conf is not None:
        assert conf.is_cuda and conf.dtype == torch.int32 and tuple(conf.shape) == (Cn, Cn) and conf.is_contiguous()
    a.loss, a.per_sample, a.weight, a.top1, a.target1, a.hits = (ptr(out[k]) for k in ("loss", "per_sample", "weight", "top1", "target1", "hits"))
    a.conf, a.saved = ptr(conf), ptr(out["saved"])
    with torch.cuda.device(dev):
        check(load().gava_soft_criterion(C.byref(a), stream_ptr(dev)), "gava_soft_criterion")
    return out


def soft_criterion_backward(logits, targets, saved, grad_loss, *, weighted=False, alpha=0.25, gamma=2.0, beta=0.0, scale=1.0):
    """dlogits [B, C] of soft_criterion's loss (the same keywords as the forward); grad_loss: the upstream gradient, a DEVICE
    fp32 scalar (never read on the host).  The targets receive no gradient."""
    a = _soft_args(logits, targets, weighted, alpha, gamma, beta, scale)
    _f32(grad_loss, "grad_loss")
    assert grad_loss.numel() == 1 and tuple(saved.shape) == (a.B, 8) and saved.is_contiguous()
    dlogits = torch.empty(a.B, a.C, dtype=torch.float32, device=logits.device)
    a.saved, a.grad_loss, a.dlogits, a.ld_dlogits = ptr(saved), ptr(grad_loss), ptr(dlogits), a.C
    with torch.cuda.device(logits.device):
        check(load().gava_soft_criterion_backward(C.byref(a), stream_ptr(logits.device)), "gava_soft_criterion_backward")
    return dlogits


def _train_head_args(kept):
    a = TrainHeadArgs()
    for k in ("video", "text", "class_offsets", "logit_scale", "logit_bias", "logits", "text_features", "video_norm", "video_inv",
              "text_norm", "text_inv", "class_mean"):
        setattr(a, k, ptr(kept.get(k)))
    a.B, a.C, a.P, a.E = kept["B"], kept["C"], kept["P"], kept["E"]
    return a


def train_head(video, text, class_offsets, logit_scale, logit_bias=None):
    """Forward of the training head (gava_train_head): raw video [B, E] and prompt features [P, E], class_offsets int32 [C+1] on
    the device (prompts of class c = rows offsets[c] .. offsets[c+1]; offsets[C] == P is the caller's promise - it is not read
    here, the kernels clamp) -> dict with logits [B, C], text_features [C, E] and what train_head_backward reuses."""
    video, text = _f32(video, "video").contiguous(), _f32(text, "text").contiguous()
    assert class_offsets.is_cuda and class_offsets.dtype == torch.int32 and class_offsets.is_contiguous() and class_offsets.dim() == 1
    B, E = video.shape
    P, Cn = text.shape[0], class_offsets.numel() - 1
    assert text.shape[1] == E and Cn >= 1
    dev = video.device
    new = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
    kept = dict(B=B, C=Cn, P=P, E=E, class_offsets=class_offsets, logit_scale=_f32(logit_scale, "logit_scale").reshape(1),
                logit_bias=_f32(logit_bias, "logit_bias").reshape(1) if logit_bias is not None else None,
                logits=new(B, Cn), text_features=new(Cn, E), video_norm=new(B, E), video_inv=new(B), text_norm=new(P, E),
                text_inv=new(P), class_mean=new(Cn, E))
    a = _train_head_args(dict(kept, video=video, text=text))
    with torch.cuda.device(dev):
        check(load().gava_train_head(C.byref(a), stream_ptr(dev)), "gava_train_head")
    return kept


def train_head_backward(kept, dlogits, dtext_features=None):
    """-> (dvideo [B, E], dtext [P, E], dlogit_scale [1], dlogit_bias [1] or None) from train_head's dict."""
    dev = dlogits.device
    new = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
    B, Cn, P, E = kept["B"], kept["C"], kept["P"], kept["E"]
    dlogits = _f32(dlogits, "dlogits").contiguous()
    assert tuple(dlogits.shape) == (B, Cn)
    if dtext_features is not None:
        dtext_features = _f32(dtext_features, "dtext_features").contiguous()
        assert tuple(dtext_features.shape) == (Cn, E)
    dvideo, dtext, dls, ws = new(B, E), new(P, E), new(1), new((B + Cn) * E)
    dlb = new(1) if kept["logit_bias"] is not None else None
    a = _train_head_args(kept)                       # (the backward reads neither the raw features nor text_features)
    a.dlogits, a.dtext_features = ptr(dlogits), ptr(dtext_features)
    a.dvideo, a.dtext, a.dlogit_scale, a.dlogit_bias, a.workspace = ptr(dvideo), ptr(dtext), ptr(dls), ptr(dlb), ptr(ws)
    with torch.cuda.device(dev):
        check(load().gava_train_head_backward(C.byref(a), stream_ptr(dev)), "gava_train_head_backward")
    return dvideo, dtext, dls, dlb


# ---- auxiliary heads and their loss terms (gava_nte_head*, gava_memory_head*, gava_sigmoid_criterion*, gava_nte_diag_loss*) ------

def _require(ok, message):
    """A caller's input is refused with GavaError, whatever the interpreter's optimisation level."""
    if not ok:
        raise GavaError(message)


def _dev32(t, what):
    """A device tensor as fp32, contiguous and 16-byte aligned (converted / copied only when it is not); CPU tensors are refused."""
    if not (torch.is_tensor(t) and t.is_cuda):
        raise GavaError(f"{what} must be a tensor on the HIP device: the auxiliary heads have no CPU fallback")
    t = t.detach()
    if t.dtype != torch.float32 or not t.is_contiguous():
        t = t.float().contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


_NTE_KEPT = ("sp_norm", "sp_inv", "nte_mean", "valid", "sim", "lm", "row_lse", "col_lse")


def _nte_args(kept):
    a = NteHeadArgs()
    for k in ("summary", "weight", "bias", "video_nte", "logit_scale", "logits_vm") + _NTE_KEPT:
        setattr(a, k, ptr(kept.get(k)))
    a.B, a.D, a.E, a.K = kept["B"], kept["D"], kept["E"], kept["K"]
    return a


def nte_head(summary, weight, bias, video_nte, logit_scale):
    """Forward of the video<->NTE head (gava_nte_head; the formulas are in include/gava_hip.h): summary [B, D], sum_proj's weight
    [E, D] and bias [E], video_nte [B, K, E], logit_scale (one element, on the device) -> dict with logits_vm [B, B] and what
    nte_head_backward reuses.  Five launches, no sync."""
    summary, weight, bias, video_nte = _dev32(summary, "summary"), _dev32(weight, "weight"), _dev32(bias, "bias"), _dev32(video_nte, "video_nte")
    _require(summary.dim() == 2 and weight.dim() == 2, "nte_head: summary and weight must have two dimensions")
    (B, D), (E, D2) = summary.shape, weight.shape
    _require(D2 == D and video_nte.dim() == 3 and video_nte.shape[0] == B and video_nte.shape[2] == E and tuple(bias.shape) == (E,),
             f"nte_head: summary {tuple(summary.shape)}, weight {tuple(weight.shape)}, bias {tuple(bias.shape)} and video_nte "
             f"{tuple(video_nte.shape)} do not fit [B, D], [E, D], [E], [B, K, E]")
    dev = summary.device
    new = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
    kept = dict(B=B, D=D, E=E, K=video_nte.shape[1], summary=summary, weight=weight, logit_scale=_dev32(logit_scale, "logit_scale").reshape(1),
                logits_vm=new(B, B), sp_norm=new(B, E), sp_inv=new(B), nte_mean=new(B, E), valid=new(B), sim=new(B, B), lm=new(B, B),
                row_lse=new(B), col_lse=new(B))
    a = _nte_args(dict(kept, bias=bias, video_nte=video_nte))
    with torch.cuda.device(dev):
        check(load().gava_nte_head(C.byref(a), stream_ptr(dev)), "gava_nte_head")
    return kept


def nte_head_backward(kept, dlogits):
    """-> (dsummary [B, D], dweight [E, D], dbias [E], dlogit_scale [1]) from nte_head's dict and d logits_vm [B, B]."""
    B, D, E = kept["B"], kept["D"], kept["E"]
    dlogits = _dev32(dlogits, "dlogits")
    _require(tuple(dlogits.shape) == (B, B), f"nte_head_backward: d logits_vm is {tuple(dlogits.shape)}, the forward's batch was {B}")
    dev = dlogits.device
    new = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
    dsummary, dweight, dbias, dls = new(B, D), new(E, D), new(E), new(1)
    ws = new(load().gava_nte_head_backward_workspace_floats(B, E))
    a = _nte_args(kept)
    a.dlogits, a.dsummary, a.dweight, a.dbias, a.dlogit_scale, a.workspace = ptr(dlogits), ptr(dsummary), ptr(dweight), ptr(dbias), ptr(dls), ptr(ws)
    with torch.cuda.device(dev):
        check(load().gava_nte_head_backward(C.byref(a), stream_ptr(dev)), "gava_nte_head_backward")
    return dsummary, dweight, dbias, dls


_MEM_KEPT = ("mem_mean", "mem_h", "mem_z", "mem_inv", "tf_h", "tf_u", "tf_inv", "cosine", "lse")


def pointer_table(params, device):
    """Device int64 tensor of the data pointers of `params` (fp32, contiguous, 16-byte aligned device tensors): the mem_params
    table of gava_memory_head.  The caller keeps `params` alive and rebuilds the table when a pointer changes."""
    for p in params:
        if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() and p.data_ptr() % 16 == 0):
            raise GavaError("memory_project's parameters must be fp32, contiguous, 16-byte aligned tensors on the HIP device")
    return torch.tensor([p.data_ptr() for p in params], dtype=torch.int64).to(device)


def _memory_args(kept):
    a = MemoryHeadArgs()
    for k in ("memory", "text_features", "tf_w1", "tf_b1", "tf_w2", "tf_b2", "mem_params", "logit_scale", "logit_bias", "logits_mt") + _MEM_KEPT:
        setattr(a, k, ptr(kept.get(k)))
    a.M, a.S, a.C, a.E = kept["M"], kept["S"], kept["C"], kept["E"]
    return a


def memory_head(memory, text_features, tf_params, mem_table, logit_scale, logit_bias=None):
    """Forward of the support-memory head (gava_memory_head): memory [M, S, E], text_features [C, E], tf_params = tf_project's
    (W1, b1, W2, b2), mem_table = pointer_table of memory_project's parameters in class order (4 per class), logit_scale and
    logit_bias one-element device tensors -> dict with logits_mt [M, C] and what memory_head_backward reuses.  Six launches."""
    memory, text_features = _dev32(memory, "memory"), _dev32(text_features, "text_features")
    tf_params = [_dev32(p, "tf_project") for p in tf_params]
    _require(memory.dim() == 3 and text_features.dim() == 2 and text_features.shape[1] == memory.shape[2],
             f"memory_head: memory {tuple(memory.shape)} and text_features {tuple(text_features.shape)} do not fit [M, S, E], [C, E]")
    M, S, E = memory.shape
    Cn = text_features.shape[0]
    H1, H2 = E // 4, E // 8
    _require(torch.is_tensor(mem_table) and mem_table.is_cuda and mem_table.dtype == torch.int64,
             "memory_head: mem_table must be a device int64 tensor (hip.pointer_table)")
    _require(mem_table.numel() == 4 * Cn, f"memory_head: text_features has {Cn} classes, the table of memory_project's parameters "
                                          f"{mem_table.numel() // 4} (4 pointers per class)")
    _require(len(tf_params) == 4 and [tuple(p.shape) for p in tf_params] == [(H1, E), (H1,), (H2, H1), (H2,)],
             f"memory_head: tf_project's parameters must be [{H1}, {E}], [{H1}], [{H2}, {H1}], [{H2}]")
    dev = memory.device
    new = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
    kept = dict(M=M, S=S, C=Cn, E=E, text_features=text_features, tf_w1=tf_params[0], tf_b1=tf_params[1], tf_w2=tf_params[2],
                tf_b2=tf_params[3], mem_params=mem_table, logit_scale=_dev32(logit_scale, "logit_scale").reshape(1),
                logit_bias=_dev32(logit_bias, "logit_bias").reshape(1) if logit_bias is not None else None,
                logits_mt=new(M, Cn), mem_mean=new(M, E), mem_h=new(Cn, M, H1), mem_z=new(Cn, M, H2), mem_inv=new(M, Cn),
                tf_h=new(Cn, H1), tf_u=new(Cn, H2), tf_inv=new(Cn), cosine=new(M, Cn), lse=new(M))
    a = _memory_args(dict(kept, memory=memory))
    with torch.cuda.device(dev):
        check(load().gava_memory_head(C.byref(a), stream_ptr(dev)), "gava_memory_head")
    return kept


def memory_head_backward(kept, dlogits, want_dtext=True):
    """-> dict(dmem_w1 [C, H1, E], dmem_b1 [C, H1], dmem_w2 [C, H2, H1], dmem_b2 [C, H2], dtf_w1, dtf_b1, dtf_w2, dtf_b2,
    dlogit_scale [1], dlogit_bias [1] or None, dtext_features [C, E] or None) from memory_head's dict and d logits_mt [M, C]."""
    M, Cn, E = kept["M"], kept["C"], kept["E"]
    H1, H2 = E // 4, E // 8
    dlogits = _dev32(dlogits, "dlogits")
    _require(tuple(dlogits.shape) == (M, Cn), f"memory_head_backward: d logits_mt is {tuple(dlogits.shape)}, the forward's was {(M, Cn)}")
    dev = dlogits.device
    new = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
    out = dict(dmem_w1=new(Cn, H1, E), dmem_b1=new(Cn, H1), dmem_w2=new(Cn, H2, H1), dmem_b2=new(Cn, H2),
               dtf_w1=new(H1, E), dtf_b1=new(H1), dtf_w2=new(H2, H1), dtf_b2=new(H2), dlogit_scale=new(1),
               dlogit_bias=new(1) if kept["logit_bias"] is not None else None,
               dtext_features=new(Cn, E) if want_dtext else None)
    ws = new(load().gava_memory_head_backward_workspace_floats(M, Cn, E))
    a = _memory_args(kept)
    a.dlogits, a.workspace = ptr(dlogits), ptr(ws)
    for k, v in out.items():
        setattr(a, k, ptr(v))
    with torch.cuda.device(dev):
        check(load().gava_memory_head_backward(C.byref(a), stream_ptr(dev)), "gava_memory_head_backward")
    return out


def _sigmoid_args(logits, labels, use_focal, alpha, gamma, scale):
    _require(torch.is_tensor(logits) and logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 2
             and (logits.shape[1] == 1 or logits.stride(1) == 1), "logits must be device fp32 [M, C] with a contiguous class dimension")
    M, Cn = logits.shape
    _require(labels.is_cuda and labels.dtype == torch.int64 and labels.is_contiguous() and tuple(labels.shape) == (M,),
             f"labels must be device int64 [{M}], contiguous")
    a = SigmoidCriterionArgs()
    a.logits, a.ld_logits, a.labels = ptr(logits), (logits.stride(0) if M > 1 else max(logits.stride(0), Cn)), ptr(labels)
    a.M, a.C, a.use_focal, a.alpha, a.gamma, a.scale = M, Cn, int(use_focal), alpha, gamma, scale
    return a


def sigmoid_criterion(logits, labels, *, use_focal=False, alpha=0.25, gamma=2.0, scale=1.0):
    """Mean over the samples of the sigmoid (focal) loss (gava_sigmoid_criterion): logits device fp32 [M, C], labels device int64
    [M] -> dict(loss (0-dim), per_sample [M], labels).  Soft targets are refused.  Two launches, no sync."""
    if not torch.is_tensor(labels) or labels.is_floating_point() or labels.dim() != 1:
        raise GavaError("gava_sigmoid_criterion takes integer class labels [M]; soft targets are not supported")
    labels = labels.to(device=logits.device, dtype=torch.int64).contiguous()
    a = _sigmoid_args(logits, labels, use_focal, alpha, gamma, scale)
    dev = logits.device
    out = dict(loss=torch.empty((), dtype=torch.float32, device=dev), per_sample=torch.empty(logits.shape[0], dtype=torch.float32, device=dev),
               labels=labels)
    a.loss, a.per_sample = ptr(out["loss"]), ptr(out["per_sample"])
    with torch.cuda.device(dev):
        check(load().gava_sigmoid_criterion(C.byref(a), stream_ptr(dev)), "gava_sigmoid_criterion")
    return out


def sigmoid_criterion_backward(logits, labels, grad_loss, *, use_focal=False, alpha=0.25, gamma=2.0, scale=1.0):
    """dlogits [M, C] of sigmoid_criterion's loss; grad_loss: the upstream gradient, a device fp32 scalar."""
    _require(grad_loss.is_cuda and grad_loss.dtype == torch.float32 and grad_loss.numel() == 1, "grad_loss must be one device fp32 value")
    a = _sigmoid_args(logits, labels, use_focal, alpha, gamma, scale)
    dlogits = torch.empty(logits.shape, dtype=torch.float32, device=logits.device)
    a.grad_loss, a.dlogits, a.ld_dlogits = ptr(grad_loss), ptr(dlogits), logits.shape[1]
    with torch.cuda.device(logits.device):
        check(load().gava_sigmoid_criterion_backward(C.byref(a), stream_ptr(logits.device)), "gava_sigmoid_criterion_backward")
    return dlogits


def nte_diag_loss(logits_vm, weight=1.0):
    """-weight * mean of the diagonal of logits_vm [B, B] (device fp32, contiguous) -> 0-dim device tensor.  One launch."""
    _require(torch.is_tensor(logits_vm) and logits_vm.is_cuda and logits_vm.dtype == torch.float32 and logits_vm.dim() == 2
             and logits_vm.shape[0] == logits_vm.shape[1] and logits_vm.is_contiguous(), "logits_vm must be device fp32 [B, B], contiguous")
    loss = torch.empty((), dtype=torch.float32, device=logits_vm.device)
    a = NteDiagArgs()
    a.logits_vm, a.B, a.weight, a.loss = ptr(logits_vm), logits_vm.shape[0], weight, ptr(loss)
    with torch.cuda.device(logits_vm.device):
        check(load().gava_nte_diag_loss(C.byref(a), stream_ptr(logits_vm.device)), "gava_nte_diag_loss")
    return loss


def nte_diag_loss_backward(B, grad_loss, weight=1.0):
    """d logits_vm [B, B] of nte_diag_loss; grad_loss: a device fp32 scalar."""
    _require(grad_loss.is_cuda and grad_loss.dtype == torch.float32 and grad_loss.numel() == 1, "grad_loss must be one device fp32 value")
    d = torch.empty(B, B, dtype=torch.float32, device=grad_loss.device)
    a = NteDiagArgs()
    a.B, a.weight, a.grad_loss, a.dlogits_vm = B, weight, ptr(grad_loss), ptr(d)
    with torch.cuda.device(d.device):
        check(load().gava_nte_diag_loss_backward(C.byref(a), stream_ptr(d.device)), "gava_nte_diag_loss_backward")
    return d
