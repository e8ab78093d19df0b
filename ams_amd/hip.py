"""ctypes binding of libams_hip.so (C ABI in include/ams_hip.h).

The product has no CPU fallback: if the library is missing or cannot be loaded, importing this module's
``lib()`` raises.  Build it with ``python -c "import __graft_entry__ as g; g.build()"`` or
``make -C ams_amd/csrc``.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

_HERE = Path(__file__).resolve().parent
LIB_PATH = _HERE / "libams_hip.so"

ABI_VERSION = 6

# enums of include/ams_hip.h
ROLE_STEM, ROLE_EXPAND, ROLE_DEPTHWISE, ROLE_PROJECT, ROLE_POOL_CONV, ROLE_ASPP, ROLE_CONCAT_PROJ, ROLE_LOGITS = range(8)
ACT_NONE, ACT_RELU, ACT_RELU6 = 0, 1, 2
DT_F32, DT_U8, DT_I32, DT_F64 = 0, 1, 3, 4          # 2 was bf16 activation storage: measured and dropped (include/ams_hip.h)
MODE_FROZEN, MODE_LIVE = 0, 1
OPT_MATMUL = 1
RESIZE_NEAREST, RESIZE_LINEAR = 0, 1
OPT_FUSE_EXPAND_DW = 2
OPT_FUSE_DW_PROJECT = 3
OPT_FUSE_FIRST_BLOCK = 4
OPT_FUSE_EXPAND_DW_STREAM = 5
OPT_FUSE_BLOCK = 6
OPT_LATE_SUBBATCH = 7
OPT_BLOCK_X6 = 8
OPT_DUAL_STREAM = 10
OPT_TRAIN_RECOMPUTE = 11
OPT_FUSE_DGRAD_BN = 16
OPT_FUSE_GEMM_RED = 17
OPT_EMULATE_BF16_STORAGE = 15
OPT_DUAL_AUTOTUNE = 12
OPT_DUAL_PARTS = 13
OPT_NAN_GRADS = 18
OPT_TRAIN_FWD_F16 = 24
OPT_SOFT_TEACHER = 25
OPT_FUSE_HEAD = 26
TLOGITS_FULL, TLOGITS_SELECTED = 0, 1          # AMS_TLOGITS_*: teacher logits [..., num_classes] / [..., K] (the student's classes, in order)
TLOGITS_LAYOUTS = {"full": TLOGITS_FULL, "selected": TLOGITS_SELECTED}
OPT_OVERLAP_WGRAD = 19
OPT_OVERLAP_HEAD = 20
OPT_STREAM_MIN_ROWS = 21
OPT_FUSE_OPERAND_BN = 22
OPT_WGRAD_FORK_EVERY = 23
MATMUL_F32, MATMUL_SPLIT_BF16, MATMUL_SPLIT_BF16_X6, MATMUL_BF16, MATMUL_SPLIT_F16 = 0, 1, 2, 3, 4
MATMUL_DEFAULT = MATMUL_SPLIT_F16      # frozen inference; the fine-tune step forms its split products on three bf16 parts in every mode but MATMUL_F32
(REGION_PARAMS, REGION_STATS, REGION_GRADS, REGION_ADAM_M, REGION_ADAM_V, REGION_FROZEN, REGION_BN_SYNC,
 REGION_LOGITS) = range(8)


class LayerDesc(C.Structure):
    _fields_ = [("role", C.c_int32), ("cin", C.c_int32), ("cout", C.c_int32), ("stride", C.c_int32),
                ("rate", C.c_int32), ("act", C.c_int32), ("residual_from", C.c_int32), ("bn_eps", C.c_float),
                ("w_off", C.c_int64), ("gamma_off", C.c_int64), ("beta_off", C.c_int64), ("mean_off", C.c_int64),
                ("var_off", C.c_int64)]


class StudentConfig(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("height", C.c_int32), ("width", C.c_int32), ("max_batch", C.c_int32),
                ("num_classes", C.c_int32), ("n_selected", C.c_int32), ("class_indices", C.c_int32 * 32),
                ("n_layers", C.c_int32), ("trainable", C.c_int32), ("act_dtype", C.c_int32),
                ("n_trainable", C.c_int64), ("n_stats", C.c_int64), ("bn_decay", C.c_float),
                ("bn_eps_frozen", C.c_float), ("pixel_scale", C.c_float)]


class DeltaVar(C.Structure):
    """ams_delta_var: one variable of a downlink delta's layout (ams_amd/delta.py builds the table)."""
    _fields_ = [("region", C.c_int32), ("reserved", C.c_int32), ("offset", C.c_int64), ("count", C.c_int64), ("mask_offset", C.c_int64)]


class RenderOut(C.Structure):
    """ams_render_out: the six views of ams_render_views, device pointers (None = not wanted), in the order of RENDER_VIEWS."""
    _fields_ = [("colour_student", C.c_void_p), ("overlay_student", C.c_void_p), ("colour_teacher", C.c_void_p), ("overlay_teacher", C.c_void_p),
                ("ignore_mask", C.c_void_p), ("cross_mask", C.c_void_p)]


class FirstBlockPlan(C.Structure):
    """ams_first_block_plan: what ams_k_first_block launched (or ams_k_first_block_plan says it would)."""
    _fields_ = [(n, C.c_int32) for n in ("out_h", "out_w", "pad_top", "pad_left", "tiles_y", "tiles_x", "ity0", "itx0", "niy", "nix",
                                         "interior_tiles", "interior_grid", "border_tiles", "border_grid", "border_walks")]


class MiningResult(C.Structure):
    """ams_mining_result: what a mined fine-tune step leaves (the k-th largest key, the valid pixels n, the rank k, the pixels kept)."""
    _fields_ = [("threshold", C.c_float), ("valid", C.c_int64), ("rank", C.c_int64), ("kept", C.c_int64)]


MINING_KEYS_OFFSET = 24832    # AMS_MINING_KEYS_OFFSET: the key map inside a mining scratch block; the mined labels follow it

RENDER_VIEWS = tuple(f[0] for f in RenderOut._fields_)
RENDER_TABLE_BYTES = 1120
CONFIDENCE_BINS = 32          # AMS_CONFIDENCE_BINS

DELTA_OK, DELTA_BAD_SIZE, DELTA_BAD_PADDING, DELTA_BAD_SCALE, DELTA_Q8_NONFINITE = 0, 1, 2, 3, 4
DELTA_MAX_VARS = 1024
# AMS_UPLINK_*: the status word of ams_uplink_encode / ams_uplink_decode
(UPLINK_OK, UPLINK_BAD_HEADER, UPLINK_BAD_TABLE, UPLINK_BAD_SLICE_END, UPLINK_BAD_POSITION, UPLINK_BAD_ZERO_LEVEL, UPLINK_BAD_LEVEL,
 UPLINK_BAD_OVERRUN, UPLINK_NO_ROOM, UPLINK_BAD_VECTOR, UPLINK_BAD_ZERO_SLICE) = range(11)

ALLREDUCE_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int32)

_vp, _i32, _i64, _f32, _sz = C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_size_t

# name -> (restype, argtypes).  Every symbol declared in include/ams_hip.h appears here; tests check both ways.
SIGNATURES = {
    "ams_last_error": (C.c_char_p, []),
    "ams_abi_version": (C.c_int, []),
    "ams_device_info": (C.c_int, [C.c_char_p, _sz, C.POINTER(_i32), C.POINTER(_i64)]),
    "ams_student_arena_bytes": (C.c_int, [C.POINTER(StudentConfig), C.POINTER(LayerDesc), C.POINTER(_sz)]),
    "ams_student_create": (C.c_int, [C.POINTER(StudentConfig), C.POINTER(LayerDesc), _vp, _sz, C.POINTER(_vp)]),
    "ams_student_destroy": (None, [_vp]),
    "ams_student_region": (C.c_int, [_vp, _i32, C.POINTER(_sz), C.POINTER(_sz)]),
    "ams_student_lowres_size": (C.c_int, [_vp, C.POINTER(_i32), C.POINTER(_i32)]),
    "ams_student_layer_tensor": (C.c_int, [_vp, _i32, _i32, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "ams_student_freeze": (C.c_int, [_vp, _vp]),
    "ams_student_predict": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _vp, _vp]),
    "ams_student_predict_with_metric": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "ams_student_predict_frames": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "ams_student_predict_frames_u8": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "ams_student_confidence": (C.c_int, [_vp, _i32, _vp, _vp, _vp, _vp, _vp]),
    "ams_student_soft_metric": (C.c_int, [_vp, _i32, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp]),
    "ams_cross_confusion": (C.c_int, [_vp, _vp, _i64, _vp, _vp]),
    "ams_cross_confusion_pairs": (C.c_int, [_vp, _vp, _i64, _i32, _i64, _vp, _vp, _i32, _vp, _vp]),
    "ams_student_soft_metric_layout": (C.c_int, [_vp, _i32, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _i32]),
    "ams_replay_pack_logits": (C.c_int, [_vp, _i32, _i32, _i32, C.POINTER(_i32), _i32, _i32, _vp, _vp]),
    "ams_replay_gather": (C.c_int, [_vp, _i64, _vp, _i64, _i32, _i32, _i32, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp]),
    "ams_replay_gather_f32": (C.c_int, [_vp, _i64, _i32, _i32, _i32, _i32, _vp, _vp, _i32, _vp, _vp]),
    "ams_replay_gather_logits": (C.c_int, [_vp, _i64, _i32, _i32, _i32, _i32, _vp, _vp, _i32, _i32, _i32, _vp, _vp]),
    "ams_replay_gather_logits_lowres": (C.c_int, [_vp, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _i32, _i32, _i32, _vp, _vp]),
    "ams_teacher_labels_from_logits": (C.c_int, [_vp, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _i64, _vp]),
    "ams_render_table_bytes": (_sz, []),
    "ams_render_views": (C.c_int, [_vp, _vp, _i32, _vp, _i32, _i32, _i32, _i32, _vp, C.POINTER(RenderOut), _vp]),
    "ams_student_train_step": (C.c_int, [_vp, _vp, _i32, _vp, _i32, _f32, _vp, _vp, _vp]),
    "ams_student_train_step_dp": (C.c_int, [_vp, _vp, _i32, _vp, _i32, _i32, _f32, _vp, _vp, ALLREDUCE_CB, _vp, _vp]),
    "ams_comm_unique_id": (C.c_int, [_vp, _sz]),
    "ams_comm_create": (C.c_int, [_vp, _sz, _i32, _i32, C.POINTER(_vp)]),
    "ams_comm_destroy": (None, [_vp]),
    "ams_comm_stats": (C.c_int, [_vp, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i64), C.POINTER(_i64)]),
    "ams_comm_set_timing": (C.c_int, [_vp, _i32]),
    "ams_comm_timing_read": (C.c_int, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(_i64)]),
    "ams_comm_allreduce": (C.c_int, [_vp, _vp, _sz, _i32, _vp]),
    "ams_student_train_step_rccl": (C.c_int, [_vp, _vp, _i32, _vp, _i32, _i32, _f32, _vp, _vp, _vp, _vp]),
    "ams_student_set_option": (C.c_int, [_vp, _i32, _i32]),
    "ams_student_feed_teacher_logits": (C.c_int, [_vp, _vp, _i32, _i32]),
    "ams_student_feed_teacher_logits_layout": (C.c_int, [_vp, _vp, _i32, _i32, _i32]),
    "ams_student_f16_fallback_layers": (C.c_int, [_vp, C.POINTER(_i32)]),
    "ams_student_set_regularizer": (C.c_int, [_vp, _vp, _i32, _f32]),
    "ams_student_set_kd": (C.c_int, [_vp, _f32, _f32]),
    "ams_student_set_loss_weights": (C.c_int, [_vp, C.POINTER(_f32), _i32, _f32]),
    "ams_student_profile": (C.c_int, [_vp, _i32]),
    "ams_student_profile_read": (C.c_int, [_vp, C.c_char_p, _sz, C.POINTER(_sz)]),
    "ams_student_get_adam_step": (C.c_int, [_vp, C.POINTER(_i64)]),
    "ams_student_set_adam_step": (C.c_int, [_vp, _i64]),
    "ams_pack_masked_fp16": (C.c_int, [_vp, _vp, _i64, _vp, _vp, _vp, _sz, _vp]),
    "ams_pack_masked_fp16_scratch": (_sz, [_i64]),
    "ams_student_apply_delta": (C.c_int, [_vp, _vp, _i64, C.POINTER(DeltaVar), _i32, _vp, _vp, _vp, _sz, _vp]),
    "ams_student_apply_delta_scratch": (_sz, [C.POINTER(DeltaVar), _i32]),
    "ams_select_changed": (C.c_int, [_vp, _vp, _i64, _i64, _vp, _vp, _sz, _vp]),
    "ams_select_changed_scratch": (_sz, [_i64]),
    "ams_select_apply": (C.c_int, [_vp, _vp, _i64, _f32, _vp, _vp, _vp]),
    "ams_student_encode_delta": (C.c_int, [_vp, _vp, C.POINTER(DeltaVar), _i32, _vp, _i64, _vp, _vp, _sz, _vp]),
    "ams_student_encode_delta_scratch": (_sz, [C.POINTER(DeltaVar), _i32]),
    "ams_student_encode_delta_q8": (C.c_int, [_vp, _vp, C.POINTER(DeltaVar), _i32, _vp, _vp, _i32, _vp, _i64, _vp, _vp, _vp, _sz, _vp]),
    "ams_student_encode_delta_q8_scratch": (_sz, [C.POINTER(DeltaVar), _i32]),
    "ams_student_apply_delta_q8": (C.c_int, [_vp, _vp, _i64, C.POINTER(DeltaVar), _i32, _vp, _vp, _vp, _sz, _vp]),
    "ams_student_apply_delta_q8_scratch": (_sz, [C.POINTER(DeltaVar), _i32]),
    "ams_uplink_max_bytes": (_i64, [_i32, _i32]),
    "ams_uplink_encode_scratch": (_sz, [_i32, _i32]),
    "ams_uplink_decode_scratch": (_sz, [_i32, _i32]),
    "ams_uplink_transform": (C.c_int, [_vp, _i32, _i32, _vp, _sz, _vp]),
    "ams_uplink_size_table": (C.c_int, [_vp, _sz, _i32, _i32, _vp, _vp]),
    "ams_uplink_encode": (C.c_int, [_vp, _sz, _i32, _i32, _i32, _vp, _i64, _vp, _vp, _vp]),
    "ams_uplink_decode": (C.c_int, [_vp, _i64, _i32, _i32, _vp, _vp, _vp, _sz, _vp]),
    "ams_uplink_inter_max_bytes": (_i64, [_i32, _i32]),
    "ams_uplink_inter_encode_scratch": (_sz, [_i32, _i32]),
    "ams_uplink_inter_decode_scratch": (_sz, [_i32, _i32]),
    "ams_uplink_inter_transform": (C.c_int, [_vp, _vp, _i32, _i32, _vp, _sz, _vp]),
    "ams_uplink_inter_size_table": (C.c_int, [_vp, _sz, _i32, _i32, _vp, _vp]),
    "ams_uplink_inter_encode": (C.c_int, [_vp, _sz, _i32, _i32, _i32, _vp, _i64, _vp, _vp, _vp]),
    "ams_uplink_inter_decode": (C.c_int, [_vp, _i64, _vp, _i32, _i32, _vp, _vp, _vp, _sz, _vp]),
    "ams_k_stem_conv": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _vp, _i32, _vp, _vp, _i32, _f32, _vp, _vp]),
    "ams_k_depthwise3x3": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _vp, _i32, _i32, _vp, _vp, _i32, _vp, _vp]),
    "ams_k_pointwise": (C.c_int, [_vp, _i64, _i32, _vp, _i32, _i32, _vp, _i64, _vp, _vp, _i32, _vp, _vp, _vp]),
    "ams_k_pointwise_split": (C.c_int, [_vp, _i64, _i32, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _sz, _vp]),
    "ams_k_pointwise_split3": (C.c_int, [_vp, _i64, _i32, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _sz, _vp]),
    "ams_k_pack_h2i": (C.c_int, [_vp, _i64, _i32, _vp, _vp]),
    "ams_k_pointwise_split_f16": (C.c_int, [_vp, _i64, _i32, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _sz, _vp, _vp, _vp]),
    "ams_k_expand_dw_stream_f16": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _sz, _i32, _i32, _vp]),
    "ams_ingest_resize_u8": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _i32, _vp, _i32, _i32, _vp]),
    "ams_k_dw_project": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "ams_k_block_fused": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _i32, _vp, _i32, _vp, _vp, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _sz, _vp]),
    "ams_k_block_fused_f16": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _i32, _vp, _i32, _vp, _vp, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _sz, _vp]),
    "ams_k_first_block_scratch": (_sz, [_i32]),
    "ams_k_first_block": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _f32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _sz,
                                    C.POINTER(FirstBlockPlan), _vp]),
    "ams_k_first_block_tiles": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _f32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ams_k_first_block_plan": (C.c_int, [_i32, _i32, _i32, _i32, _i32, C.POINTER(_i32), C.POINTER(FirstBlockPlan)]),
    "ams_k_expand_dw_steps": (C.c_int, [_i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, C.POINTER(_i32), _sz]),
    "ams_k_expand_dw": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _i32, _vp, _i32, _i32, _vp, _vp, _vp, _vp]),
    "ams_k_expand_dw_stream": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _sz, _i32, _i32, _vp]),
    "ams_k_global_mean": (C.c_int, [_vp, _i32, _i64, _i32, _vp, _vp, _sz, _vp]),
    "ams_k_global_mean_scratch": (_sz, [_i32, _i32]),
    "ams_k_upsample_argmax": (C.c_int, [_vp, _i32, _i32, _i32, _i32, C.POINTER(_i32), _i32, _i32, _i32, _vp, _vp, _vp,
                                        _vp, _vp]),
    "ams_k_upsample_confidence": (C.c_int, [_vp, _i32, _i32, _i32, _i32, C.POINTER(_i32), _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "ams_confidence_stats_len": (_sz, []),
    "ams_k_upsample_soft_metric": (C.c_int, [_vp, _i32, _i32, _i32, _i32, C.POINTER(_i32), _i32, _i32, _i32, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp]),
    "ams_k_upsample_soft_metric_layout": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _i32, C.POINTER(_i32), _i32, _i32, _i32, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "ams_soft_metric_stats_len": (_sz, [_i32]),
    "ams_k_ce_grad": (C.c_int, [_vp, _i32, _i32, _i32, _i32, C.POINTER(_i32), _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "ams_k_ce_loss_grad": (C.c_int, [_vp, _i32, _i32, _i32, _i32, C.POINTER(_i32), _i32, _i32, _i32, _vp, _vp, _vp, _vp, _sz, _vp]),
    "ams_k_ce_loss_grad_scratch": (_sz, [_i32, _i32, _i32, _i32]),
    "ams_k_ce_loss_grad_soft": (C.c_int, [_vp, _i32, _i32, _i32, _i32, C.POINTER(_i32), _i32, _i32, _i32, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _sz, _vp]),
    "ams_k_ce_loss_grad_soft_layout": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _i32, C.POINTER(_i32), _i32, _i32, _i32, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _sz, _vp]),
    "ams_k_ce_loss_grad_kd": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _i32, C.POINTER(_i32), _i32, _i32, _i32, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _sz, _vp,
                                        _f32, _f32]),
    "ams_k_ce_loss_grad_weighted": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _i32, C.POINTER(_i32), _i32, _i32, _i32, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _sz,
                                              _vp, _f32, _f32, C.POINTER(_f32), _f32]),
    "ams_k_ce_loss_grad_mined": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _i32, C.POINTER(_i32), _i32, _i32, _i32, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _sz,
                                           _vp, _f32, _f32, C.POINTER(_f32), _f32, _f32, _vp, _vp, _vp, _vp, _sz]),
    "ams_k_loss_mining_scratch": (_sz, [_i32, _i32, _i32]),
    "ams_student_set_loss_mining": (C.c_int, [_vp, _f32, _vp, _sz]),
    "ams_student_mining_result": (C.c_int, [_vp, _vp, _vp]),
    "ams_debug_launch_table_needs_attr": (C.c_int, [_i32, C.c_uint64, _sz]),
    "ams_debug_reload_knobs": (C.c_int, []),
    "ams_debug_phase_cycles": (C.c_int, [C.c_int32, C.POINTER(C.c_uint64), C.c_int32]),
    "ams_k_pointwise_wgrad": (C.c_int, [_vp, _vp, _i64, _i32, _i32, _vp, _vp, _sz, _vp]),
    "ams_k_pointwise_wgrad_scratch": (_sz, [_i64, _i32, _i32]),
    "ams_k_pointwise_wgrad_split": (C.c_int, [_vp, _vp, _i64, _i32, _i32, _vp, _vp, _sz, _vp]),
    "ams_k_depthwise3x3_dgrad": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _vp, _i32, _i32, _vp, _vp]),
    "ams_k_depthwise3x3_wgrad": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _sz, _vp]),
    "ams_k_pointwise_xform": (C.c_int, [_vp, _i64, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "ams_k_pointwise_wgrad_xform": (C.c_int, [_vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "ams_k_pointwise_red": (C.c_int, [_vp, _i64, _i32, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _sz,
                                     C.POINTER(_i32), _vp, _sz, _vp]),
    "ams_k_depthwise3x3_fwd_bn_scratch": (_sz, [_i32, _i32, _i32, _i32, _i32]),
    "ams_k_depthwise3x3_fwd_bn": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _sz, C.POINTER(_i32), _vp]),
    "ams_k_depthwise3x3_dgrad_bn_scratch": (_sz, [_i32, _i32, _i32, _i32]),
    "ams_k_depthwise3x3_dgrad_bn": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _sz,
                                             C.POINTER(_i32), _vp]),
    "ams_k_depthwise3x3_fwd_bn_tiles_scratch": (_sz, [_i32, _i32, _i32, _i32, _i32]),
    "ams_k_depthwise3x3_fwd_bn_tiles": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _sz, C.POINTER(_i32), _vp]),
    "ams_k_depthwise3x3_dgrad_bn_apply_scratch": (_sz, [_i32, _i32, _i32, _i32, _i32]),
    "ams_k_depthwise3x3_dgrad_bn_apply": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _sz,
                                                    C.POINTER(_i32), _vp]),
    "ams_k_xx_gram_scratch": (_sz, [_i64, _i32]),
    "ams_k_xx_gram": (C.c_int, [_vp, _i64, _i32, _vp, _sz, _vp, _vp, _vp]),
    "ams_k_expand_stats": (C.c_int, [_vp, _i32, _vp, _i32, C.c_double, _vp, _vp, _vp, _f32, _f32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ams_k_xdw_train_scratch": (_sz, [_i32, _i32, _i32, _i32, _i32]),
    "ams_k_xdw_fwd_stats": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _vp, _i32, _vp, _vp, _sz, C.POINTER(_i32), C.POINTER(_i64), _vp]),
    "ams_k_xdw_bwd_reduce": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _i32, _vp, _vp, _sz,
                                      C.POINTER(_i32), C.POINTER(_i64), _vp]),
    "ams_k_xdw_bwd_dx": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _vp, _i32, _vp, _vp, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ams_k_xdw_stem_scratch": (_sz, [_i32, _i32, _i32]),
    "ams_k_xdw_bwd_reduce_stem": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _f32, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _sz,
                                           C.POINTER(_i32), C.POINTER(_i64), _vp]),
    "ams_k_xdw_dwe": (C.c_int, [_vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ams_k_col_plan": (C.c_int, [_i64, _i32, _i32, C.POINTER(_i32)]),
    "ams_k_colstats_scratch": (_sz, [_i64, _i32]),
    "ams_k_colstats": (C.c_int, [_vp, _i64, _i32, _vp, _vp, _vp, _sz, _vp]),
    "ams_k_colstats_f64": (C.c_int, [_vp, _i64, _i32, _vp, _vp, _vp]),
    "ams_k_bn_finalize": (C.c_int, [_vp, C.c_double, _i32, _vp, _vp, _vp, _f32, _f32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ams_k_colstats_bn": (C.c_int, [_vp, _i64, _i32, _vp, _vp, _vp, _sz, C.c_double, _vp, _vp, _f32, _f32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ams_k_bn_fwd_partials": (C.c_int, [_vp, _i32, _i64, _i32, _vp, C.c_double, _vp, _vp, _vp, _f32, _f32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ams_k_bn_bwd_partials": (C.c_int, [_vp, _i32, _i64, _i32, _vp, C.c_double, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ams_k_partials_to_sums": (C.c_int, [_vp, _i32, _i64, _i32, _vp, _vp]),
    "ams_k_bn_bwd_reduce": (C.c_int, [_vp, _vp, _i64, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _sz, _vp]),
    "ams_k_bn_bwd_coef": (C.c_int, [_vp, C.c_double, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ams_k_bn_param_grads": (C.c_int, [_vp, _i32, _vp, _vp, _vp]),
    "ams_k_bn_bwd_reduce_coef": (C.c_int, [_vp, _vp, _i64, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _sz, C.c_double, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ams_k_bn_act": (C.c_int, [_vp, _i64, _i32, _vp, _vp, _i32, _vp, _vp, _vp]),
    "ams_k_bn_bwd_apply": (C.c_int, [_vp, _vp, _i64, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp]),
    "ams_k_bn_fold": (C.c_int, [_vp, _vp, _vp, _vp, _f32, _i32, _vp, _vp, _vp]),
    "ams_k_reduce_splits": (C.c_int, [_vp, _i32, _i64, _i64, _vp, _vp]),
    "ams_k_reduce_batch": (C.c_int, [C.POINTER(_vp), C.POINTER(_i32), C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_vp), _i32, _vp]),
    "ams_k_colsum_scratch": (_sz, [_i32]),
    "ams_k_colsum": (C.c_int, [_vp, _i64, _i32, _i32, _vp, _vp, _sz, _vp]),
    "ams_k_image_colsum_scratch": (_sz, [_i32, _i32]),
    "ams_k_image_colsum": (C.c_int, [_vp, _i32, _i64, _i32, _i32, _vp, _vp, _sz, _vp]),
    "ams_k_l2_regularizer": (C.c_int, [_vp, _vp, _vp, _i64, _i32, _f32, _vp, _sz, _vp, _vp]),
    "ams_k_adam": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i64, _f32, _f32, _f32, _f32, _vp]),
}

_lib = None


class AmsHipError(RuntimeError):
    pass


def lib() -> C.CDLL:
    """Load libams_hip.so once; raise (never fall back) when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    path = Path(os.environ.get("AMS_HIP_LIB", str(LIB_PATH)))
    if not path.exists():
        raise AmsHipError(
            "HIP library %s not found: the AMS student has no CPU fallback. Build it with "
            "`make -C ams_amd/csrc` (hipcc --offload-arch=gfx950)." % path)
    # libams_hip.so needs libamdhip64.so.7; PyTorch-ROCm bundles its own copy under the same soname.  Whichever is
    # loaded first serves both, and device pointers are only valid inside one runtime instance: load torch first.
    import torch  # noqa: F401
    handle = C.CDLL(str(path))
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(handle, name)          # AttributeError here = header/library mismatch: fail loudly
        fn.restype = res
        fn.argtypes = args
    if handle.ams_abi_version() != ABI_VERSION:
        raise AmsHipError("libams_hip.so ABI %d, binding expects %d" % (handle.ams_abi_version(), ABI_VERSION))
    _lib = handle
    return handle


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = lib().ams_last_error()
        raise AmsHipError("%s failed (%d): %s" % (what or "libams_hip call", rc, msg.decode() if msg else "?"))
