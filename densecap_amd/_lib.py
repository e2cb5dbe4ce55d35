"""ctypes binding of libdensecap_hip.so (the C ABI declared in include/densecap.h; measurement / test hooks in
include/densecap_debug.h).

There is deliberately NO fallback: if the shared library has not been built
(`python -c "import __graft_entry__ as g; g.build()"` or `make -C densecap_amd/csrc`)
importing the product path raises, and if no HIP device is present dc_create fails.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# DENSECAP_HIP_LIB: another build of the same library (the LuaJIT binding honours the same variable)
LIB_PATH = os.environ.get("DENSECAP_HIP_LIB") or os.path.join(_HERE, "lib", "libdensecap_hip.so")

DC_NUM_VGG_CONVS = 13
c_float_p = C.POINTER(C.c_float)
c_int32_p = C.POINTER(C.c_int32)


class DcWeights(C.Structure):
    _fields_ = ([("conv_w", c_float_p * DC_NUM_VGG_CONVS), ("conv_b", c_float_p * DC_NUM_VGG_CONVS)] +
                [(n, c_float_p) for n in (
                    "rpn_conv_w", "rpn_conv_b", "rpn_box_w", "rpn_box_b", "rpn_score_w", "rpn_score_b",
                    "fc6_w", "fc6_b", "fc7_w", "fc7_b", "obj_w", "obj_b", "boxreg_w", "boxreg_b",
                    "lm_enc_w", "lm_enc_b", "lm_emb", "lstm_w", "lstm_b", "lm_out_w", "lm_out_b", "anchors")] +
                [("field_centers", C.c_float * 4)] +
                [(n, C.c_int32) for n in ("num_anchors", "rpn_hidden", "vocab_size", "seq_length", "enc_size",
                                          "rnn_size", "fc_dim")])


class DcResult(C.Structure):
    _fields_ = [("capacity", C.c_int32), ("K", C.c_int32), ("T", C.c_int32),
                ("boxes", c_float_p), ("scores", c_float_p), ("tokens", c_int32_p)]


DC_BOXES_CLIP = 1


class DcBoxList(C.Structure):
    _fields_ = [("boxes", c_float_p), ("n", C.c_int32), ("src", c_int32_p)]


class DcSampleOpts(C.Structure):
    _fields_ = [("num_samples", C.c_int32), ("temperature", C.c_float), ("seed", C.c_uint64)]


class DcSampleTrunc(C.Structure):
    """dc_sample_trunc: {0, 1.0} = no truncation."""
    _fields_ = [("top_k", C.c_int32), ("top_p", C.c_float)]


class DcBeamState(C.Structure):
    """dc_beam_state (include/densecap_debug.h): device pointers to the nprop x beam state rows of the beam search."""
    _fields_ = [("h", C.c_void_p), ("c", C.c_void_p), ("beam_lp", C.c_void_p), ("beams", C.c_void_p), ("tok", C.c_void_p),
                ("parent", C.c_void_p), ("fin", C.c_void_p)]


class DcBeamOpts(C.Structure):
    """dc_beam_opts: the standard beam search of dc_beam_captions / dc_op_lm_beam_n."""
    _fields_ = [("beam_size", C.c_int32), ("n_best", C.c_int32), ("length_alpha", C.c_float)]


class DcLocalizeOpts(C.Structure):
    """dc_localize_opts: the per-query NMS of dc_localize_captions."""
    _fields_ = [("nms_thresh", C.c_float), ("max_regions", C.c_int32), ("min_objectness", C.c_float)]


class DcLossOpts(C.Structure):
    """dc_loss_opts: the settings of the training forward (the sampler's and the five loss weights)."""
    _fields_ = [("batch_size", C.c_int32), ("high_thresh", C.c_float), ("low_thresh", C.c_float), ("remove_outbounds", C.c_int32),
                ("mid_box_reg_weight", C.c_float), ("mid_objectness_weight", C.c_float), ("end_box_reg_weight", C.c_float),
                ("end_objectness_weight", C.c_float), ("captioning_weight", C.c_float), ("seed", C.c_uint64)]


class DcSamplerForced(C.Structure):
    """dc_sampler_forced: host lists of ranks that take the place of the sampler's draws."""
    _fields_ = [("pos_sample_idx", c_int32_p), ("num_pos", C.c_int32), ("neg_sample_idx", c_int32_p), ("num_neg", C.c_int32)]


class DcLosses(C.Structure):
    """dc_losses: the six validation losses of one image and the sampler's counts."""
    _fields_ = ([(n, C.c_double) for n in ("mid_objectness_loss", "mid_box_reg_loss", "end_objectness_loss", "end_box_reg_loss",
                                           "captioning_loss", "total_loss")] +
                [(n, C.c_int32) for n in ("num_pos", "num_neg", "total_pos", "total_neg", "masked_mid", "masked_end", "flags")])


class DcLossDump(C.Structure):
    """dc_loss_dump: host buffers (batch_size int32 each) for the sampler's three lists."""
    _fields_ = [("pos_input_idx", c_int32_p), ("pos_target_idx", c_int32_p), ("neg_input_idx", c_int32_p)]


class DcLmGrads(C.Structure):
    """dc_lm_grads: device buffers for the gradients of dc_op_lm_grad, in the layouts of dc_weights; codes may be null."""
    _fields_ = [(n, C.c_void_p) for n in ("lm_enc_w", "lm_enc_b", "lm_emb", "lstm_w", "lstm_b", "lm_out_w", "lm_out_b", "codes")]


class DcRecogGrads(C.Structure):
    """dc_recog_grads: device buffers for the gradients of dc_op_recog_grad, in checkpoint layouts; all required."""
    _fields_ = [(n, C.c_void_p) for n in ("fc6_w", "fc6_b", "fc7_w", "fc7_b", "obj_w", "obj_b", "boxreg_w", "boxreg_b", "feat",
                                          "roi_boxes")]


class DcRpnGrads(C.Structure):
    """dc_rpn_grads: device buffers for the RPN's gradients, in checkpoint layouts, and a feature-map gradient; all required."""
    _fields_ = [(n, C.c_void_p) for n in ("rpn_conv_w", "rpn_conv_b", "rpn_box_w", "rpn_box_b", "rpn_score_w", "rpn_score_b", "feat")]


class DcCnnGrads(C.Structure):
    """dc_cnn_grads: device buffers for the gradients of conv3_1 .. conv5_3 (OIHW) and their biases; x may be null."""
    _fields_ = [("conv_w", C.c_void_p * 9), ("conv_b", C.c_void_p * 9), ("x", C.c_void_p)]


class DcCnnDump(C.Structure):
    """dc_cnn_dump: optional device buffers for what dc_op_cnn_grad's forward kept and the masked gradients."""
    _fields_ = [("act", C.c_void_p * 9), ("prepool", C.c_void_p * 2), ("feat", C.c_void_p), ("dy", C.c_void_p * 9)]


class DcTrainOpts(C.Structure):
    """dc_train_opts: Adam's settings and the L2 weight decay (train_opts.lua's defaults: 1e-5, 0.9, 0.999, 1e-8, 1e-6)."""
    _fields_ = [(n, C.c_double) for n in ("learning_rate", "beta1", "beta2", "epsilon", "weight_decay")]


class DcBeamStdState(C.Structure):
    """dc_beam_std_state (include/densecap_debug_beam.h): dc_beam_state plus len."""
    _fields_ = DcBeamState._fields_ + [("len", C.c_void_p)]


class DcStepGemm(C.Structure):
    """dc_step_gemm (include/densecap_debug_step.h): one GEMM of a decode step on the caller's device operands."""
    _fields_ = [("A", C.c_void_p), ("W", C.c_void_p), ("bias", C.c_void_p), ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32),
                ("plan_M", C.c_int32), ("epilogue", C.c_int32), ("relu", C.c_int32), ("C", C.c_void_p), ("ldc", C.c_int32),
                ("part_ld", C.c_int32), ("part", C.c_void_p), ("part_idx", C.c_void_p), ("rowidx", C.c_void_p), ("t", C.c_int32),
                ("inv_temp", C.c_float), ("seed", C.c_uint64), ("amax_cols", C.c_int32), ("amax_n", C.c_int32),
                ("m_dev_or_null", C.c_void_p)]


class DcStepTail(C.Structure):
    """dc_step_tail (include/densecap_debug_step.h): one launch of one row tail on the caller's partials and state."""
    _fields_ = [("kind", C.c_int32), ("nslots", C.c_int32), ("ld", C.c_int32), ("xg_rows", C.c_int32), ("part", C.c_void_p),
                ("part_idx", C.c_void_p), ("xg", C.c_void_p), ("gates_pre", C.c_void_p), ("c", C.c_void_p), ("h", C.c_void_p),
                ("n", C.c_int32), ("Hd", C.c_int32), ("n_dev_or_null", C.c_void_p), ("zero_c", C.c_int32), ("fixed_tok", C.c_int32),
                ("tgt", C.c_void_p), ("end_tok", C.c_int32), ("T", C.c_int32), ("t", C.c_int32), ("acc", C.c_void_p),
                ("fin", C.c_void_p), ("seq", C.c_void_p)]


class DcGlueRoiPool(C.Structure):
    """dc_glue_roi_pool (include/densecap_debug_glue.h): one launch of the group form of bilinear RoI pooling."""
    _fields_ = [("feat_hwc", C.c_void_p), ("feat_stride", C.c_size_t), ("nimg", C.c_int32), ("h", C.c_int32), ("w", C.c_int32),
                ("C", C.c_int32), ("boxes", C.c_void_p), ("B", C.c_int32), ("B_dev", C.c_void_p), ("bdev_stride", C.c_int32),
                ("pick", C.c_void_p), ("src_boxes", C.c_void_p), ("src_stride", C.c_size_t), ("src_rows", C.c_int32),
                ("img_h", C.c_int32), ("img_w", C.c_int32), ("HH", C.c_int32), ("WW", C.c_int32), ("out", C.c_void_p),
                ("out_layout", C.c_int32)]


class DcGlueFinalPack(C.Structure):
    """dc_glue_final_pack (include/densecap_debug_glue.h): one launch of the group's result records."""
    _fields_ = [("final_boxes", C.c_void_p), ("obj", C.c_void_p), ("tokens", C.c_void_p), ("tok_gather", C.c_int32),
                ("codes", C.c_void_p), ("picks", C.c_void_p), ("count", C.c_void_p), ("count_stride", C.c_int32),
                ("fault", C.c_void_p), ("nimg", C.c_int32), ("P", C.c_int32), ("T", C.c_int32), ("D", C.c_int32),
                ("pack", C.c_void_p), ("stride", C.c_size_t), ("box_src", C.c_void_p)]


class DenseCapError(RuntimeError):
    pass


_SIGS = {
    "dc_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int]),
    "dc_destroy": (None, [C.c_void_p]),
    "dc_last_error": (C.c_char_p, [C.c_void_p]),
    "dc_load_weights": (C.c_int, [C.c_void_p, C.POINTER(DcWeights)]),
    "dc_set_test_args": (C.c_int, [C.c_void_p, C.c_float, C.c_float, C.c_int]),
    "dc_set_localization_test_args": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_int]),
    "dc_set_lanes": (C.c_int, [C.c_void_p, C.c_int]),
    "dc_set_caption_order": (C.c_int, [C.c_void_p, C.c_int]),
    "dc_preprocess_size": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "dc_preprocess_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "dc_set_math_mode": (C.c_int, [C.c_void_p, C.c_int]),
    "dc_set_graph_replay": (C.c_int, [C.c_void_p, C.c_int]),
    "dc_set_beam_size": (C.c_int, [C.c_void_p, C.c_int]),
    "dc_set_group": (C.c_int, [C.c_void_p, C.c_int]),
    "dc_forward_test": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(DcResult)]),
    "dc_forward_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(DcResult)]),
    "dc_forward_images": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int,
                                    C.c_int, C.POINTER(DcResult)]),
    "dc_extract_features": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                      C.c_void_p, c_int32_p]),
    "dc_extract_features_images": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                             C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, c_int32_p]),
    "dc_forward_boxes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(DcBoxList), C.c_int,
                                   C.POINTER(DcResult)]),
    "dc_forward_boxes_images": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int,
                                          C.c_int, C.POINTER(DcBoxList), C.c_int, C.POINTER(DcResult)]),
    "dc_extract_features_boxes": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                            C.c_int, C.c_int, C.POINTER(DcBoxList), C.c_int, C.c_int, C.c_void_p,
                                            C.c_void_p, c_int32_p]),
    "dc_stage_times": (C.c_int, [C.c_void_p, C.POINTER(C.c_char_p), c_float_p, C.c_int]),
    "dc_mfma_profile": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_double),
                                  C.POINTER(C.c_double)]),
    "dc_debug_fetch": (C.c_int64, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64]),
    "dc_debug_set": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int64]),
    "dc_debug_plan_gemm": (C.c_int, [C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int, c_int32_p]),
    "dc_debug_beam_topk": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                     C.c_void_p]),
    "dc_debug_beam_merge": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                      C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "dc_debug_beam_start": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(DcBeamState), C.c_void_p, C.c_void_p]),
    "dc_debug_beam_step": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(DcBeamState), C.POINTER(DcBeamState), C.c_void_p,
                                     C.c_void_p]),
    "dc_debug_screen_scores": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "dc_debug_rescore_tail": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p]),
    "dc_comm_unique_id": (C.c_int, [C.c_void_p]),
    "dc_comm_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    "dc_comm_create_ex": (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "dc_comm_transport": (C.c_char_p, [C.c_void_p]),
    "dc_comm_destroy": (None, [C.c_void_p]),
    "dc_comm_last_error": (C.c_char_p, [C.c_void_p]),
    "dc_gather_results": (C.c_int, [C.c_void_p, C.POINTER(DcResult), C.c_int, C.POINTER(DcResult)]),
    "dc_malloc": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_size_t]),
    "dc_free": (C.c_int, [C.c_void_p, C.c_void_p]),
    "dc_memcpy_h2d": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "dc_memcpy_d2h": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "dc_synchronize": (C.c_int, [C.c_void_p]),
    "dc_op_chw_to_hwc": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "dc_op_hwc_to_chw": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "dc_op_pack_conv3x3_weights": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    "dc_op_conv3x3": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                C.c_int, C.c_int, C.c_int, C.c_int]),
    "dc_op_conv3x3_relu_pool": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                          C.c_int, C.c_int]),
    "dc_op_conv3x3_c3": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                   C.c_int, C.c_int]),
    "dc_op_maxpool2x2_ceil": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]),
    "dc_op_linear": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                               C.c_int, C.c_int]),
    "dc_op_make_anchors": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float,
                                     C.c_float, C.c_void_p, C.c_int]),
    "dc_op_apply_box_transform": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "dc_op_clip_boxes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_float,
                                   C.c_float, C.c_float]),
    "dc_op_xcycwh_to_x1y1x2y2": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "dc_op_box_iou": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "dc_op_rpn_decode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_float,
                                   C.c_float, C.c_float, C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "dc_op_nms": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_int,
                            C.c_void_p, C.c_void_p]),
    "dc_op_bilinear_roi_pool": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                          C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]),
    "dc_op_lm_sample": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "dc_op_lm_score": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "dc_score_captions": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                    C.POINTER(DcResult), C.c_void_p]),
    "dc_sample_captions": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(DcSampleOpts),
                                     C.POINTER(DcResult), C.c_void_p, C.c_void_p]),
    "dc_op_lm_sample_n": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(DcSampleOpts), C.c_void_p,
                                    C.c_void_p]),
    "dc_sample_captions_trunc": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(DcSampleOpts),
                                           C.POINTER(DcSampleTrunc), C.POINTER(DcResult), C.c_void_p, C.c_void_p, C.c_void_p]),
    "dc_op_lm_sample_n_trunc": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(DcSampleOpts),
                                          C.POINTER(DcSampleTrunc), C.c_void_p, C.c_void_p, C.c_void_p]),
    "dc_beam_captions": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(DcBeamOpts), C.POINTER(DcResult),
                                   C.c_void_p, C.c_void_p]),
    "dc_op_lm_beam_n": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(DcBeamOpts), C.c_void_p, C.c_void_p]),
    "dc_op_nms_multi": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_int,
                                  C.c_void_p, C.c_void_p]),
    "dc_op_eval_match": (C.c_int, [C.c_void_p] + [C.c_void_p] * 5 + [C.c_int, C.c_float, C.c_int] + [C.c_void_p] * 7),
    "dc_op_box_sampler": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(DcLossOpts),
                                    C.POINTER(DcSamplerForced)] + [C.c_void_p] * 6),
    "dc_forward_losses": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                    C.POINTER(DcLossOpts), C.POINTER(DcSamplerForced), C.POINTER(DcLosses), C.POINTER(DcLossDump)]),
    "dc_op_lm_grad": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_float, C.POINTER(DcLmGrads),
                                C.POINTER(C.c_double), C.c_void_p]),
    "dc_op_roi_pool_grad": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p] + [C.c_int] * 5 +
                            [C.c_void_p] * 3),
    "dc_op_recog_grad": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                   C.c_int, C.c_int, C.POINTER(DcLossOpts), C.POINTER(DcRecogGrads), C.POINTER(C.c_double),
                                   C.POINTER(C.c_double), c_int32_p]),
    "dc_loss_gradients": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                    C.POINTER(DcLossOpts), C.POINTER(DcSamplerForced), C.POINTER(DcLosses), C.POINTER(DcLossDump),
                                    C.POINTER(DcRecogGrads), C.POINTER(DcLmGrads)]),
    "dc_feature_size": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "dc_op_conv3x3_grad": (C.c_int, [C.c_void_p] + [C.c_void_p] * 3 + [C.c_int] * 4 + [C.c_void_p] * 3),
    "dc_op_maxpool2x2_grad": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p]),
    "dc_op_relu_grad": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong]),
    "dc_set_dropout": (C.c_int, [C.c_void_p, C.c_float]),
    "dc_get_dropout": (C.c_int, [C.c_void_p, c_float_p]),
    "dc_op_dropout": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_uint64]),
    "dc_op_relu_dropout_grad": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_float]),
    "dc_op_cnn_grad": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(DcCnnGrads), C.POINTER(DcCnnDump)]),
    "dc_op_rpn_grad": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                 C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.POINTER(DcLossOpts), C.c_float,
                                 C.POINTER(DcRpnGrads), C.POINTER(C.c_double), C.POINTER(C.c_double), c_int32_p]),
    "dc_forward_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                      C.POINTER(DcLossOpts), C.POINTER(DcSamplerForced), C.POINTER(DcLosses), C.POINTER(DcLossDump),
                                      C.POINTER(DcRecogGrads), C.POINTER(DcLmGrads), C.c_float, C.POINTER(DcRpnGrads)]),
    "dc_forward_backward_cnn": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                          C.POINTER(DcLossOpts), C.POINTER(DcSamplerForced), C.POINTER(DcLosses), C.POINTER(DcLossDump),
                                          C.POINTER(DcRecogGrads), C.POINTER(DcLmGrads), C.c_float, C.POINTER(DcRpnGrads),
                                          C.POINTER(DcCnnGrads)]),
    "dc_train_begin": (C.c_int, [C.c_void_p, C.POINTER(DcTrainOpts)]),
    "dc_train_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                C.POINTER(DcLossOpts), C.POINTER(DcSamplerForced), C.POINTER(DcLosses), C.POINTER(DcLossDump), C.c_float]),
    "dc_train_set_cnn": (C.c_int, [C.c_void_p, C.c_int]),
    "dc_train_end": (C.c_int, [C.c_void_p]),
    "dc_get_weights": (C.c_int, [C.c_void_p, C.POINTER(DcWeights)]),
    "dc_op_adam": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(DcTrainOpts)]),
    "dc_train_set_grad_clip": (C.c_int, [C.c_void_p, C.c_double]),
    "dc_train_grad_norm": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), c_float_p]),
    "dc_op_grad_norm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                  c_float_p]),
    "dc_train_get_state": (C.c_int, [C.c_void_p, C.POINTER(DcWeights), C.POINTER(DcWeights), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "dc_train_set_state": (C.c_int, [C.c_void_p, C.POINTER(DcWeights), C.POINTER(DcWeights), C.c_int, C.c_int]),
    "dc_localize_captions": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                       C.POINTER(DcLocalizeOpts), C.POINTER(DcResult), C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p]),
}
# the hook of include/densecap_debug_sample.h (bound like the others; the two lists above mirror densecap.h / densecap_debug.h)
_SAMPLE_HOOK_SIGS = {
    "dc_debug_sample_trunc_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_uint64,
                                             C.c_float, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p]),
}
# the hooks of include/densecap_debug_step.h (the classic decode step's GEMM epilogues and row tails; bound like the others)
_STEP_HOOK_SIGS = {
    "dc_debug_step_gemm": (C.c_int, [C.c_void_p, C.POINTER(DcStepGemm)]),
    "dc_debug_step_tail": (C.c_int, [C.c_void_p, C.POINTER(DcStepTail)]),
}
# the hooks of include/densecap_debug_beam.h (the standard beam search; bound like the others)
_BEAM_STD_HOOK_SIGS = {
    "dc_debug_beam_std_merge": (C.c_int, [C.c_void_p] + [C.c_void_p] * 6 + [C.c_int] * 5 + [C.c_void_p] * 6),
    "dc_debug_beam_std_finish": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                           C.c_float, C.c_void_p, C.c_void_p]),
    "dc_debug_beam_std_start": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(DcBeamStdState), C.c_void_p,
                                          C.c_void_p]),
    "dc_debug_beam_std_step": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(DcBeamStdState),
                                         C.POINTER(DcBeamStdState), C.c_void_p, C.c_void_p]),
}
# the hooks of include/densecap_debug_grad.h (the language model's backward kernels; bound like the others)
_GRAD_HOOK_SIGS = {
    "dc_debug_wgrad": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "dc_debug_embed_segsum": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "dc_debug_softmax_grad": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_void_p]),
    "dc_debug_lstm_cell_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                         C.c_void_p, C.c_void_p]),
    "dc_debug_lm_grad_stage_ms": (C.c_int, [C.c_void_p, c_float_p]),
}
# the hooks of include/densecap_debug_recog.h (the recognition net's backward kernels; bound like the others)
_RECOG_HOOK_SIGS = {
    "dc_debug_roi_tap_index": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int] * 7 + [C.c_void_p] * 4),
    "dc_debug_end_crit_grad": (C.c_int, [C.c_void_p] + [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_float, C.c_float] + [C.c_void_p] * 4),
    "dc_debug_heads_bwd": (C.c_int, [C.c_void_p] + [C.c_void_p] * 5 + [C.c_int] * 3 + [C.c_void_p] * 3),
    "dc_debug_permute_fc6_back": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "dc_debug_recog_grad_stage_ms": (C.c_int, [C.c_void_p, c_float_p]),
}
# the hooks of include/densecap_debug_bwd.h (the backward kernels on the operand forms production uses; bound like the others)
_BWD_HOOK_SIGS = {
    "dc_debug_wgrad_ld": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                    C.c_int]),
    "dc_debug_colsum": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "dc_debug_lstm_cell_bwd_ex": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 5 +
                                  [C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
}
# the hooks of include/densecap_debug_rpn.h (the RPN backward's kernels; bound like the others)
_RPN_HOOK_SIGS = {
    "dc_debug_conv3x3_wgrad": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 5 + [C.c_void_p]),
    "dc_debug_rpn_dheads": (C.c_int, [C.c_void_p] + [C.c_void_p] * 4 + [C.c_int] * 3 + [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                      C.c_void_p, C.c_int, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_void_p]),
    "dc_debug_rpn_heads_bwd": (C.c_int, [C.c_void_p] + [C.c_void_p] * 3 + [C.c_int] * 3 + [C.c_void_p]),
    "dc_debug_rpn_grad_kept": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, c_float_p]),
}
# the hooks of include/densecap_debug_optim.h (the optimiser's kernels; bound like the others)
_OPTIM_HOOK_SIGS = {
    "dc_debug_adam_multi": (C.c_int, [C.c_void_p] + [C.POINTER(C.c_void_p)] * 4 + [C.POINTER(C.c_size_t), C.c_int, C.c_int,
                                                                                   C.POINTER(DcTrainOpts), C.c_int]),
    "dc_debug_screen_operands": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "dc_debug_unpack_conv3x3": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
}
# the hook of include/densecap_debug_clip.h (gradient clipping: the norm pass and the scaled Adam launch; bound like the others)
_CLIP_HOOK_SIGS = {
    "dc_debug_adam_multi_clip": (C.c_int, [C.c_void_p] + [C.POINTER(C.c_void_p)] * 4 +
                                 [C.POINTER(C.c_size_t), C.c_int, C.c_int, C.POINTER(DcTrainOpts), C.c_int, C.c_double,
                                  C.POINTER(C.c_double), c_float_p]),
}
# the hooks of include/densecap_debug_glue.h (the forward path's glue kernels, one launch each; bound like the others)
_GLUE_HOOK_SIGS = {
    "dc_debug_boxes_ingest": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 5 + [C.c_void_p] * 3 + [C.c_int]),
    "dc_debug_roi_pool_group": (C.c_int, [C.c_void_p, C.POINTER(DcGlueRoiPool)]),
    "dc_debug_recog_heads": (C.c_int, [C.c_void_p] + [C.c_void_p] * 8 + [C.c_int, C.c_int]),
    "dc_debug_iota_count": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "dc_debug_gather_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                       C.c_int]),
    "dc_debug_survivor_compact": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p, C.c_void_p]),
    "dc_debug_final_pack": (C.c_int, [C.c_void_p, C.POINTER(DcGlueFinalPack)]),
}
# the hooks of include/densecap_debug_nms.h (the two NMS launchers with a device-side row count; bound like the others)
_NMS_HOOK_SIGS = {
    "dc_debug_nms": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_int,
                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "dc_debug_nms_multi": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_int,
                                     C.c_void_p, C.c_void_p]),
}

EXPORTED_SYMBOLS = tuple(_SIGS)
_lib = None


def lib():
    """Load libdensecap_hip.so (once) and attach the prototypes.  Raises if it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise DenseCapError(
                "libdensecap_hip.so not built at %s -- run `make -C densecap_amd/csrc` "
                "(there is no CPU fallback)" % LIB_PATH)
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in (list(_SIGS.items()) + list(_SAMPLE_HOOK_SIGS.items()) + list(_STEP_HOOK_SIGS.items()) +
                                  list(_BEAM_STD_HOOK_SIGS.items()) +
                                  list(_GRAD_HOOK_SIGS.items()) + list(_RECOG_HOOK_SIGS.items()) +
                                  list(_BWD_HOOK_SIGS.items()) + list(_RPN_HOOK_SIGS.items()) + list(_OPTIM_HOOK_SIGS.items()) +
                                  list(_CLIP_HOOK_SIGS.items()) +
                                  list(_GLUE_HOOK_SIGS.items()) + list(_NMS_HOOK_SIGS.items())):
            fn = getattr(l, name)  # AttributeError if the symbol is not exported
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib


def check(ctx, rc, what=""):
    if rc < 0:
        msg = lib().dc_last_error(ctx)
        raise DenseCapError("%s failed (%d): %s" % (what or "densecap call", rc,
                                                    msg.decode() if msg else "?"))
    return rc
