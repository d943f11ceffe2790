"""ctypes binding of libsloika_amd.so (the C ABI declared in include/sloika_amd.h).

There is NO CPU fallback: if the HIP library is missing or no GPU is visible, every compute entry point
raises.  (The library itself loads fine on a CPU-only box, which is what the symbol-export test uses.)
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
#: SLOIKA_AMD_LIB: another build of the same C ABI (tools/build_diag_lib.sh: the diagnostic build the scripts under tools/ use)
LIB_PATH = os.environ.get("SLOIKA_AMD_LIB") or os.path.join(_HERE, "_build", "libsloika_amd.so")

SLK_OK = 0
SLK_ERR_INVALID_ARG = -1
SLK_ERR_UNSUPPORTED = -2
SLK_ERR_LAUNCH = -3
SLK_ERR_WORKSPACE = -4
SLK_ERR_NO_DEVICE = -5
SLK_GRU_STACK_MAX = 8          # include/sloika_amd.h: layers per slk_gru_bar16_stack_f32 launch
SLK_GRU_STACK_NO_LENS = 2      # ... bit of a layer's `reverse`: the layer ignores the ragged lengths


class GruStackLayer(C.Structure):
    """slk_gru_stack_layer of include/sloika_amd.h."""
    _fields_ = [("x", C.c_void_p), ("ldx", C.c_long), ("h_out", C.c_void_p), ("ldh", C.c_long), ("pack", C.c_void_p),
                ("reverse", C.c_int), ("reserved", C.c_int)]


class ViterbiPlan(C.Structure):
    """slk_viterbi_plan of include/sloika_amd.h (slk_viterbi_kmer_plan: what the stand-alone decoder launches for a shape)."""
    _fields_ = [("kernel", C.c_int), ("blank_steps", C.c_int), ("staged_rows", C.c_int), ("tb_row_bytes", C.c_int),
                ("walker_rows", C.c_int), ("walker_dma", C.c_int)]

POST_RAW, POST_PLAIN, POST_LOG, POST_LN = 0, 1, 2, 3
VIT_KERNEL_GENERIC, VIT_KERNEL_WORKGROUP4, VIT_KERNEL_WAVE4 = 0, 1, 2

_vp, _i, _l, _f, _sz, _d = C.c_void_p, C.c_int, C.c_long, C.c_float, C.c_size_t, C.c_double

# name -> (restype, argtypes); mirrors include/sloika_amd.h one to one
PROTOTYPES = {
    "slk_abi_version": (_i, []),
    "slk_error_string": (C.c_char_p, [_i]),
    "slk_device_count": (_i, []),
    "slk_clock_probe": (_i, [_vp, _i, _vp]),
    "slk_selftest_mfma4_f32": (_i, [_vp, _vp, _vp, _i, _i, _vp]),
    "slk_med_mad_normalise_f32": (_i, [_vp, _i, _i, _vp, _l, _l, _vp, _vp, _vp]),
    "slk_med_mad_normalise_ragged_f32": (_i, [_vp, _i, _l, _vp, _vp, _l, _l, _vp, _vp, _vp]),
    "slk_window_std_f32": (_i, [_vp, _i, _i, _vp, _vp]),
    "slk_event_features_f32": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _vp, C.c_int64, _i, _i, _vp, _vp, C.c_int64, _vp]),
    "slk_conv1d_out_len": (_i, [_i, _i, _i, _i, _i]),
    "slk_conv1d_f32": (_i, [_vp, _l, _l, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "slk_window_f32": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "slk_gemm_bias_act_f32": (_i, [_vp, _l, _vp, _vp, _vp, _l, _l, _i, _i, _i, _vp]),
    "slk_linear_softmax_f32": (_i, [_vp, _l, _vp, _vp, _vp, _l, _i, _i, _vp]),
    "slk_linear_rowstats_f32": (_i, [_vp, _l, _vp, _vp, _vp, _l, _l, _i, _i, _vp, _vp]),
    "slk_pack_reads_f32": (_i, [_vp, _vp, _vp, _i, _vp, _l, _vp]),
    "slk_reads_nonfinite_f32": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp]),
    "slk_adc_to_pa_i16": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp]),
    "slk_open_pore_trim_f32": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "slk_split_f16x2_f32": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp]),
    "slk_linear_rowstats_f16x3": (_i, [_vp, _l, _vp, _vp, _vp, _vp, _vp, _l, _l, _i, _i, _vp, _vp]),
    "slk_pack_bf16x3_bytes": (_sz, [_i, _i]),
    "slk_pack_bf16x3_f32": (_i, [_vp, _i, _i, _vp, _vp]),
    "slk_gemm_bias_act_bf16x6": (_i, [_vp, _l, _vp, _vp, _vp, _l, _l, _i, _i, _i, _vp]),
    "slk_gemm_dact_bf16x6": (_i, [_vp, _l, _vp, _vp, _l, _i, _vp, _l, _l, _i, _i, _vp]),
    "slk_gemm_bias_act_f16x3": (_i, [_vp, _l, _vp, _vp, _vp, _vp, _vp, _l, _l, _i, _i, _i, _vp]),
    "slk_softmax_from_stats_f32": (_i, [_vp, _l, _vp, _vp, _l, _l, _i, _vp]),
    "slk_softmax_rows_f32": (_i, [_vp, _l, _i, _vp]),
    "slk_softmax_rowstats_f32": (_i, [_vp, _l, _i, _vp, _vp]),
    "slk_viterbi_kmer_logits_f32": (_i, [_vp, _l, _vp, _i, _i, _i, _i, _f, _f, _vp, _sz, _vp, _vp, _vp, _vp]),
    "slk_viterbi_kmer_logits_ragged_f32": (_i, [_vp, _l, _vp, _i, _i, _i, _i, _f, _f, _vp, _vp, _sz, _vp, _vp, _vp, _vp]),
    "slk_softmax_viterbi_pack_bytes": (_sz, [_i, _i, _i]),
    "slk_softmax_viterbi_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "slk_softmax_viterbi_pack_f32": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp]),
    "slk_softmax_viterbi_f32": (_i, [_vp, _l, _vp, _i, _i, _i, _i, _i, _f, _f, _vp, _i, _vp, _sz, _vp, _vp, _vp, _vp, _vp]),
    "slk_gru_recurrent_ragged_f32": (_i, [_vp, _vp, _vp, _vp, _l, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "slk_gru_scan16_f32": (_i, [_vp, _l, _vp, _vp, _vp, _l, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "slk_log_post_logits_f32": (_i, [_vp, _l, _vp, _vp, _sz, _i, _f, _vp]),
    "slk_gru_recurrent_f32": (_i, [_vp, _vp, _vp, _vp, _l, _i, _i, _i, _i, _i, _i, _vp]),
    "slk_gru_recurrent_f32_ex": (_i, [_vp, _vp, _vp, _vp, _l, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "slk_gru_workspace_bytes": (_sz, [_i, _i, _i]),
    "slk_gru_f32": (_i, [_vp, _l, _vp, _vp, _vp, _vp, _vp, _l, _i, _i, _i, _i, _i, _i, _i, _vp, _sz, _vp]),
    "slk_paths_to_bases": (_i, [_vp, _l, _vp, _i, _i, _i, _i, C.c_ulonglong, _vp, _l, _vp, _vp]),
    "slk_gru_bar16_pack_bytes": (_sz, [_i, _i]),
    "slk_gru_bar16_pack_f32": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp]),
    "slk_gru_bar16_stack_f32": (_i, [_i, _vp, _i, _i, _i, _i, _vp, _vp]),
    "slk_gru_bar16_stack_path": (_i, [_i, _i]),
    "slk_gru_bar16_f32": (_i, [_vp, _l, _vp, _vp, _vp, _vp, _vp, _l, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "slk_lstm_recurrent_f32": (_i, [_vp, _vp, _vp, _vp, _l, _i, _i, _i, _i, _i, _i, _vp]),
    "slk_lstm_recurrent_ragged_f32": (_i, [_vp, _vp, _vp, _vp, _l, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "slk_lstm_workspace_bytes": (_sz, [_i, _i, _i]),
    "slk_lstm_f32": (_i, [_vp, _l, _vp, _vp, _vp, _vp, _vp, _l, _i, _i, _i, _i, _i, _i, _i, _vp, _sz, _vp]),
    "slk_viterbi_kmer_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "slk_viterbi_kmer_plan": (_i, [_i, _i, _i, _i, _i, C.POINTER(ViterbiPlan)]),
    "slk_viterbi_kmer_f32": (_i, [_vp, _i, _i, _i, _i, _f, _i, _f, _vp, _sz, _vp, _vp, _vp, _vp]),
    "slk_viterbi_marginals_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "slk_viterbi_marginals_f32": (_i, [_vp, _i, _i, _i, _i, _f, _i, _f, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "slk_viterbi_marginals_ckpt_workspace_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "slk_viterbi_marginals_ckpt_f32": (_i, [_vp, _i, _i, _i, _i, _f, _i, _f, _vp, _i, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "slk_paths_to_bases_qual": (_i, [_vp, _l, _vp, _vp, _l, _vp, _i, _i, _i, _i, _i, C.c_ulonglong, _vp, _vp, _l, _vp, _vp]),
    "slk_log_post_f32": (_i, [_vp, _vp, _sz, _i, _f, _vp]),
    "slk_prepare_post_f32": (_i, [_vp, _vp, _sz, _f, _vp]),
    "slk_argmax_decode_f32": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    "slk_prepare_post_drop_bad_f32": (_i, [_vp, _i, _i, _i, _i, _f, _vp, _vp, _vp, _vp, _vp]),
    "slk_estimate_transitions_f64": (_i, [_vp, _i, _i, _i, _i, _i, _d, _d, _d, _d, _vp, _vp, _vp, _vp]),
    "slk_decode_profile_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "slk_decode_profile_f64": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _d, _vp, _vp, _sz, _vp, _vp, _vp, _vp]),
    "slk_slip_update_f32": (_i, [_vp, _i, _f, _vp, _vp, _vp]),
    "slk_map_to_sequence_workspace_bytes": (_sz, [_i, _i]),
    "slk_map_to_sequence_f32": (_i, [_vp, _i, _i, _vp, _i, _f, _vp, _vp, _vp, _sz, _vp, _vp, _vp]),
    "slk_map_to_sequence_batch_f32": (_i, [_vp, _i, _vp, _vp, _vp, _i, _i, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "slk_map_to_sequence_long_workspace_bytes": (_sz, [_i, _i, _i]),
    "slk_map_to_sequence_long_f32": (_i, [_vp, _i, _i, _vp, _i, _f, _vp, _vp, _vp, _sz, _i, _vp, _vp, _vp]),
    "slk_map_to_sequence_long_batch_f32": (_i, [_vp, _i, _vp, _vp, _vp, _i, _i, _f, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp]),
    "slk_kmer_labels_i32": (_i, [_vp, _l, _i, _i, C.c_char_p, _i, _i, _vp, _vp, _vp]),
    "slk_raw_chunk_labels_workspace_bytes": (_sz, [_l]),
    "slk_raw_chunk_labels_i32": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _l, _i, _i, _vp, _sz, _vp, _vp]),
    "slk_raw_chunk_labels_interp_i32": (_i, [_vp, _vp, _vp, _l, _i, _i, _l, _vp, _l, _i, C.c_char_p, _i, _l, _i, _vp, _i, _vp, _vp,
                                             _vp, _vp]),
    "slk_remap_pack_log_post_f32": (_i, [_vp, _l, _l, _i, _i, _i, _vp, _vp, _f, _vp, _vp]),
    "slk_event_remap_labels_i32": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, C.c_int64, _vp, _vp, _vp, _vp]),
    "slk_lstm_fused16_f32": (_i, [_vp, _l, _vp, _vp, _vp, _vp, _vp, _l, _i, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "slk_lstm_scan16_f32": (_i, [_vp, _vp, _vp, _vp, _l, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "slk_activation_f32": (_i, [_vp, _vp, _sz, _i, _vp]),
    "slk_train_pack_xh_f32": (_i, [_vp, _l, _vp, _l, _vp, _i, _i, _i, _i, _i, _vp]),
    "slk_train_pack_xrh_f32": (_i, [_vp, _vp, _vp, _l, _i, _i, _vp]),
    "slk_gru_backward_f32": (_i, [_vp, _l, _vp, _l, _vp, _vp, _l, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "slk_gru_backward16_f32": (_i, [_vp, _l, _vp, _l, _vp, _vp, _l, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "slk_gru_backward16_dx_f32": (_i, [_vp, _l, _vp, _l, _vp, _vp, _l, _vp, _vp, _vp, _vp, _vp, _vp, _l, _i, _i, _i, _i, _i, _i, _i, _vp, _l, _i,
                                       _vp]),
    "slk_lstm_gates_f32": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "slk_lstm_backward_f32": (_i, [_vp, _l, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "slk_lstm_backward16_f32": (_i, [_vp, _l, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "slk_softmax_xent_grad_f32": (_i, [_vp, _l, _vp, _vp, _vp, _i, _i, _i, _i, _f, _vp, _vp, _vp]),
    "slk_softmax_seq_grad_f32": (_i, [_vp, _l, _vp, _vp, _l, _vp, _vp, _i, _i, _i, _f, _vp]),
    "slk_linear_xent_grad_f16x3": (_i, [_vp, _l, _vp, _vp, _vp, _vp, _vp, _l, _i, _i, _vp, _vp, _i, _i, _i, _f, _vp, _vp, _vp, _vp]),
    "slk_reduce_sum_f32": (_i, [_vp, _sz, _i, _vp, _vp]),
    "slk_reduce_rows_sum_f32": (_i, [_vp, _i, _sz, _vp, _vp, _vp]),
    "slk_linear_xent_eval_f16x3": (_i, [_vp, _l, _vp, _vp, _vp, _vp, _i, _i, _vp, _i, _i, _vp, _vp, _vp]),
    "slk_softmax_xent_eval_f32": (_i, [_vp, _l, _vp, _vp, _i, _i, _i, _vp, _vp, _vp]),
    "slk_reduce_rows_sum_i32": (_i, [_vp, _sz, _vp, _vp]),
    "slk_gemm_tn_workspace_bytes": (_sz, [_l, _i, _i]),
    "slk_gemm_tn_f32": (_i, [_vp, _l, _vp, _l, _vp, _l, _l, _i, _i, _vp, _vp, _sz, _vp]),
    "slk_gemm_tn_bf16x6_f32": (_i, [_vp, _l, _vp, _l, _vp, _l, _l, _i, _i, _vp, _vp, _sz, _vp]),
    "slk_gemm_tn_multi_workspace_bytes": (_sz, [_l, _i, _vp, _vp]),
    "slk_gemm_tn_multi_bf16x6_f32": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _vp, _l, _vp, _vp, _vp, _vp, _sz, _vp]),
    "slk_act_backward_f32": (_i, [_vp, _vp, _vp, _sz, _i, _vp]),
    "slk_add_inplace_f32": (_i, [_vp, _vp, _sz, _vp]),
    "slk_train_im2col_cin1_f32": (_i, [_vp, _l, _l, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "slk_train_im2col_f32": (_i, [_vp, _l, _i, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "slk_train_col2im_f32": (_i, [_vp, _i, _i, _i, _i, _i, _i, _i, _vp, _l, _vp]),
    "slk_adamski_update_f32": (_i, [_vp, _vp, _vp, _vp, _sz, _f, _f, _f, _f, _f, _f, _f, _f, _vp]),
    "slk_sgd_update_f32": (_i, [_vp, _vp, _vp, _sz, _f, _f, _f, _f, _f, _vp]),
    "slk_align_pass_width": (_i, []),
    "slk_align_local_workspace_bytes": (_sz, [_i, _i, _i]),
    "slk_align_local_batch_u8": (_i, [_vp, _l, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "slk_revcomp_u8": (_i, [_vp, _vp, _i, _l, _vp, _vp]),
    "slk_align_traceback_max_band": (_i, []),
    "slk_align_traceback_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "slk_align_traceback_batch_u8": (_i, [_vp, _l, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _sz, _vp, _vp, _sz, _vp, _vp]),
    "slk_align_error_profile_u8": (_i, [_vp, _l, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp]),
    "slk_forward_score_max_positions": (_i, []),
    "slk_forward_score_batch_f32": (_i, [_vp, _l, _vp, _l, _vp, _i, _vp, _vp, _i, _i, _i, _i, _f, _vp, _vp]),
    "slk_forward_score_batch_f64": (_i, [_vp, _l, _vp, _l, _vp, _i, _vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "slk_forward_backward_workspace_bytes": (_sz, [_i, _vp, _vp]),
    "slk_forward_backward_batch_f32": (_i, [_vp, _l, _vp, _l, _vp, _i, _vp, _vp, _i, _i, _i, _i, _f, _vp, _vp, _l, _vp, _vp, _vp, _sz,
                                            _vp]),
    "slk_forward_backward_batch_f64": (_i, [_vp, _l, _vp, _l, _vp, _i, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _l, _vp, _vp, _vp, _sz, _vp]),
    "slk_rescore_edits_max_new": (_i, []),
    "slk_rescore_edits_workspace_bytes": (_sz, [_i, _vp, _vp]),
    "slk_rescore_edits_batch_f32": (_i, [_vp, _l, _vp, _l, _vp, _i, _vp, _vp, _i, _i, _i, _f, _vp, _vp, _vp, _vp, _vp, C.c_int64, _vp,
                                         _vp, _vp, _sz, _vp]),
    "slk_rescore_edits_batch_f64": (_i, [_vp, _l, _vp, _l, _vp, _i, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, C.c_int64, _vp, _vp,
                                         _vp, _sz, _vp]),
    "slk_rescore_band_max_width": (_i, []),
    "slk_rescore_edits_banded_workspace_bytes": (_sz, [_i, _vp, _i]),
    "slk_rescore_edits_banded_batch_f32": (_i, [_vp, _l, _vp, _l, _vp, _i, _vp, _vp, _i, _i, _f, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp,
                                                C.c_int64, _vp, _vp, _vp, _sz, _vp]),
    "slk_rescore_edits_banded_batch_f64": (_i, [_vp, _l, _vp, _l, _vp, _i, _vp, _vp, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp,
                                                C.c_int64, _vp, _vp, _vp, _sz, _vp]),
    "slk_genome_kmer_keys_u8": (_i, [_vp, _vp, _i, _l, _i, _vp, _vp, _vp]),
    "slk_genome_seed_workspace_bytes": (_sz, [_i, _i, _l, _i]),
    "slk_genome_seed_votes_u8": (_i, [_vp, _l, _vp, _i, _i, _vp, _i, _l, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "slk_genome_windows_u8": (_i, [_vp, _l, _vp, _vp, _vp, _vp, _i, _l, _vp, _vp]),
    "slk_pileup_columns_u8": (_i, [_vp, _l, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _l, _i, _i, _vp, _vp, _vp]),
    "slk_pileup_count_u8": (_i, [_vp, _l, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _l, _i, _l, _l, _i, _vp, _vp, _vp]),
    "slk_pileup_call_u8": (_i, [_vp, _vp, _vp, _l, _l, _l, _i, _i, _vp, _vp, _vp, _vp]),
    "slk_pileup_count_qual_u8": (_i, [_vp, _l, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _l, _i, _l, _l, _i, _vp, _vp, _vp, _vp,
                                      _vp, _vp]),
    "slk_pileup_call_qual_u8": (_i, [_vp, _vp, _vp, _vp, _vp, _l, _l, _l, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "slk_polish_read_windows": (_i, [_vp, _l, _vp, _vp, _l, _i, _vp, _vp, _l, _vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _l, _i, _i,
                                     _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "slk_letter_edits_count": (_i, [_vp, _vp, _vp, _i, _l, _i, _i, _i, _vp, _vp, _vp]),
    "slk_letter_edits_emit": (_i, [_vp, _l, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, C.c_int64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "slk_letter_edits_new": (_i, [_vp, _l, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, C.c_int64, _vp, _vp, C.c_int64, _vp, _vp]),
    "slk_polish_window_kmers": (_i, [_vp, _l, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, C.c_int64, _vp, _vp]),
    "slk_polish_sum_gains_f64": (_i, [_vp, _i, _vp, _vp, _vp, _vp, C.c_int64, C.c_int64, C.c_int64, _vp, _vp, _vp]),
    "slk_variant_edits_count": (_i, [_vp, _l, _vp, _i, _vp, _vp, _vp, _vp, _vp, C.c_int64, C.c_int64, _vp, _vp, _vp, _i, _i, _i, _vp, _vp,
                                     _vp, _vp]),
    "slk_variant_edits_emit": (_i, [_vp, _l, _vp, _vp, _vp, _vp, _vp, C.c_int64, C.c_int64, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp,
                                    C.c_int64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "slk_variant_edits_new": (_i, [_vp, _l, _vp, _vp, _vp, _vp, _vp, C.c_int64, C.c_int64, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i,
                                   C.c_int64, _vp, _vp, _vp, _vp, C.c_int64, _vp, _vp]),
    "slk_polish_sum_variant_gains_f64": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, C.c_int64, C.c_int64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "slk_repeat_variants_count": (_i, [_vp, _l, _vp, _i, C.c_int64, C.c_int64, _i, _i, _i, _i, _vp, _vp, _vp]),
    "slk_repeat_variants_emit": (_i, [_vp, _l, _vp, _i, C.c_int64, C.c_int64, _i, _i, _i, _i, _vp, _vp, C.c_int64, C.c_int64, _vp, _vp,
                                      _vp, _vp, _vp, _vp]),
    "slk_pileup_alleles_count": (_i, [_vp, _vp, _vp, _l, _vp, _i, C.c_int64, C.c_int64, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "slk_pileup_alleles_emit": (_i, [_vp, _vp, _vp, _l, _vp, _i, C.c_int64, C.c_int64, _i, _i, _i, _i, _i, _i, _vp, _vp, C.c_int64,
                                     C.c_int64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "slk_variant_genotypes_f64": (_i, [_vp, _i, _vp, _vp, _vp, _vp, C.c_int64, C.c_int64, _d, _vp, _vp, _vp]),
}

_lib = None


class SloikaAmdError(RuntimeError):
    pass


def lib():
    """Load the HIP library; fail loudly when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise SloikaAmdError(
                "sloika_amd: HIP extension %s is missing. Build it with `python -m sloika_amd.build` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback." % LIB_PATH)
        # torch first: it ships its own HIP runtime, and if this library's dependency on libamdhip64 is resolved before
        # torch has loaded its copy, torch.cuda.is_available() turns False for the rest of the process (seen on the GPU
        # box when a script touched the library before importing torch)
        import torch  # noqa: F401
        handle = C.CDLL(LIB_PATH)
        for name, (res, args) in PROTOTYPES.items():
            fn = getattr(handle, name)          # AttributeError here = header/library mismatch
            fn.restype = res
            fn.argtypes = args
        if handle.slk_abi_version() != 1:
            raise SloikaAmdError("sloika_amd: ABI version mismatch")
        _lib = handle
    return _lib


def error_string(code):
    return lib().slk_error_string(code).decode()


def check(rc, what=""):
    if rc == SLK_OK:
        return
    msg = "%s: %s (code %d)" % (what or "sloika_amd", error_string(rc), rc)
    if rc == SLK_ERR_INVALID_ARG:
        raise ValueError(msg)            # the reference asserts on these (layers.py:152-155, decode.py:50-52)
    raise SloikaAmdError(msg)


def require_gpu():
    """Raise unless a HIP device is usable through both the library and torch."""
    import torch
    if lib().slk_device_count() < 1 or not torch.cuda.is_available():
        raise SloikaAmdError("sloika_amd: no AMD GPU visible; the basecalling path only runs on the HIP kernels "
                             "(no CPU fallback)")
    return True
