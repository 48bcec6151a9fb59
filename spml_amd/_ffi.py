"""ctypes binding of libspml_hip.so (include/spml_hip.h).

Torch is plumbing only: it owns device memory and the HIP stream; every call
below passes raw `data_ptr()`s and `torch.cuda.current_stream().cuda_stream` to
the C-ABI.  There is no CPU fallback: if the library is missing or a tensor is
not on a GPU the call raises."""
import ctypes
import functools
import os
import threading
from ctypes import c_char_p, c_double, c_float, c_int, c_int64, c_size_t, c_void_p

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# SPML_HIP_LIB: load another build of the same library (A/B timing of kernel variants)
LIB_PATH = os.environ.get('SPML_HIP_LIB') or os.path.join(_HERE, 'lib', 'libspml_hip.so')

_lib = None
_lock = threading.Lock()

# name -> (restype, argtypes); mirrors include/spml_hip.h one to one.
_P = c_void_p
_SIGNATURES = {
    'spml_status_string': (c_char_p, [c_int]),
    'spml_abi_version': (c_int, []),
    'spml_normalize_concat_loc_f32': (c_int, [_P, c_int, c_int, c_int, c_int, _P, _P, _P, _P, _P]),
    'spml_normalize_concat_loc_bwd_f32': (c_int, [_P, c_int, c_int, c_int, c_int, _P, _P, _P, _P, _P, _P]),
    'spml_normalize_concat_local_f32': (c_int, [_P, c_int, c_int, c_int, c_int, _P, c_int, _P, _P, _P, _P]),
    'spml_normalize_concat_local_nhwc_supported': (c_int, [c_int, c_int]),
    'spml_normalize_concat_local_nhwc_f32': (c_int, [_P, c_int, c_int, c_int, c_int, _P, c_int, _P, _P, _P, _P]),
    'spml_normalize_concat_local_nhwc_bwd_f32': (c_int, [_P, c_int, c_int, c_int, c_int, _P, c_int, _P, _P, _P,
                                                         _P, _P]),
    'spml_normalize_concat_local_bwd_f32': (c_int, [_P, c_int, c_int, c_int, c_int, _P, c_int, _P, _P, _P,
                                                    _P, _P]),
    'spml_normalize_rows_f32': (c_int, [_P, c_int64, c_int, _P, _P]),
    'spml_normalize_rows_bwd_f32': (c_int, [_P, _P, c_int64, c_int, _P, _P]),
    'spml_kmeans_init_grid_i64': (c_int, [c_int, c_int, c_int, c_int, _P, _P]),
    'spml_relabel_unique_workspace_bytes': (c_size_t, [c_int64]),
    'spml_relabel_unique_i64': (c_int, [_P, c_int64, _P, _P, c_int64, _P, _P, c_size_t, _P]),
    'spml_kmeans_workspace_bytes': (c_size_t, [c_int64, c_int, c_int, c_int, c_int64]),
    'spml_kmeans_run_f32': (c_int, [_P, c_int64, c_int, _P, c_int, c_int64, c_int, _P, c_int, _P, _P,
                                    c_int, _P, c_size_t, _P]),
    'spml_kmeans_assign_f32': (c_int, [_P, c_int64, c_int, _P, c_int, c_int64, c_int, _P, _P, c_int,
                                       _P, c_size_t, _P]),
    'spml_kmeans_fused_pass_f32': (c_int, [_P, c_int64, c_int, _P, c_int, c_int64, c_int, _P, _P, _P,
                                           c_int, _P, c_size_t, _P]),
    'spml_kmeans_preconvert_f32': (c_int, [_P, c_int64, c_int, _P, c_int, c_int64, c_int, _P, c_size_t,
                                           _P]),
    'spml_kmeans_path_name': (c_char_p, [c_int64, c_int, c_int, c_int, c_int64, c_int, c_int, c_int]),
    'spml_kmeans_profile_layout': (c_int, [c_int64, c_int, c_int, c_int, c_int64, c_int, _P, _P]),
    'spml_kmeans_run_profiled_f32': (c_int, [_P, c_int64, c_int, _P, c_int, c_int64, c_int, _P, c_int,
                                             _P, c_int, _P, c_size_t, _P, c_size_t, _P]),
    'spml_segment_sum_normalize_f32': (c_int, [_P, _P, c_int64, c_int, c_int64, _P, _P, _P]),
    'spml_segment_sum_normalize_bwd_f32': (c_int, [_P, _P, _P, c_int64, c_int, c_int64, _P, _P, c_int, _P]),
    'spml_segment_sum_det_workspace_bytes': (c_size_t, [c_int64, c_int]),
    'spml_segment_sum_normalize_det_f32': (c_int, [_P, _P, c_int64, c_int, c_int64, _P, _P, _P, c_size_t, _P]),
    'spml_set_deterministic': (c_int, [c_int]),
    'spml_get_deterministic': (c_int, []),
    'spml_build_experiment': (c_int, []),
    'spml_segsort_nll_workspace_bytes': (c_size_t, [c_int64, c_int64, c_int]),
    'spml_segsort_nll_fwd_f32': (c_int, [_P, _P, _P, c_int64, _P, _P, c_int64, c_int, c_float, c_int,
                                         _P, _P, _P, c_size_t, _P]),
    'spml_segsort_nll_bwd_f32': (c_int, [_P, _P, _P, c_int64, _P, _P, c_int64, c_int, c_float, c_int,
                                         _P, _P, _P, _P, c_int64, _P, c_size_t, _P]),
    'spml_segsort_nll_path_name': (c_int, [c_int64, c_int64, c_int, c_int, c_int, c_int64, _P, c_size_t]),
    'spml_segsort_nll_batched_supported': (c_int, [c_int, c_int]),
    'spml_segsort_nll_batched_workspace_bytes': (c_size_t, [c_int, _P, _P, c_int]),
    'spml_segsort_nll_batched_fwd_f32': (c_int, [_P, _P, _P, _P, _P, _P, _P, c_int, c_int, c_float, c_int,
                                                 _P, _P, _P, c_size_t, _P]),
    'spml_segsort_nll_batched_bwd_f32': (c_int, [_P, _P, _P, _P, _P, _P, _P, c_int, c_int, c_float, c_int,
                                                 _P, _P, _P, _P, _P, c_size_t, _P]),
    'spml_topk_workspace_bytes': (c_size_t, [c_int64, c_int64, c_int, c_int]),
    'spml_topk_affinity_f32': (c_int, [_P, c_int64, _P, c_int64, c_int, c_int, _P, _P, _P, c_float,
                                       _P, _P, _P, c_size_t, _P]),
    'spml_affinity_workspace_bytes': (c_size_t, [c_int, c_int, c_int64]),
    'spml_affinity_transition_f32': (c_int, [_P, c_int, c_int, c_int64, c_float, c_int, _P, _P, c_size_t,
                                             _P]),
    'spml_bn_workspace_bytes': (c_size_t, [c_int64, c_int]),
    'spml_bn_act_fwd_f32': (c_int, [_P, _P, c_int64, c_int, _P, _P, _P, _P, c_float, c_float, c_int, _P, _P, _P,
                                    _P, c_size_t, _P]),
    'spml_bn_act_bwd_f32': (c_int, [_P, _P, _P, c_int64, c_int, _P, _P, _P, _P, _P, _P, _P, _P, c_size_t, _P]),
    'spml_hl8_from_f32': (c_int, [_P, c_int64, c_int, _P, c_int, _P, _P]),
    'spml_hl8_weight_transposed_f32': (c_int, [_P, c_int, c_int, c_int, _P, _P, _P]),
    'spml_conv_hl8_supported': (c_int, [c_int, c_int, c_int]),
    'spml_conv_hl8_f32': (c_int, [_P, _P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, _P]),
    'spml_conv_hl8_stats_layout': (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, _P, _P]),
    'spml_conv_hl8_stats_f32': (c_int, [_P, _P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, _P]),
    'spml_bn_fwd_hl8_chunks_f32': (c_int, [_P, _P, c_int, c_int, _P, _P, c_int64, c_int, _P, _P, _P, _P, c_float, c_float,
                                           c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    'spml_conv_hl8_bwd_stats_layout': (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, _P, _P]),
    'spml_conv_hl8_bwd_stats_f32': (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int,
                                            c_int, c_int, _P]),
    'spml_conv_hl8_bwd_stats_addend_f32': (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int,
                                                   c_int, c_int, c_int, _P, _P, _P]),
    'spml_bn_bwd_hl8_chunks_f32': (c_int, [_P, _P, _P, _P, c_int, c_int, c_int64, c_int, _P, _P, _P, _P, _P, _P, _P, _P,
                                           _P, _P, _P, _P, _P]),
    'spml_bn_act_bwd_reduce_ext_chunks_f32': (c_int, [_P, c_int, c_int, c_int64, c_int, _P, _P, _P, _P, _P]),
    'spml_conv_wgrad_hl8_supported': (c_int, [c_int, c_int, c_int]),
    'spml_conv_wgrad_workspace_bytes': (c_size_t, [c_int, c_int, c_int, c_int, c_int, c_int]),
    'spml_conv_wgrad_hl8_f32': (c_int, [_P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, _P,
                                        c_size_t, _P]),
    'spml_conv_wgrad_pyramid_hl8_supported': (c_int, [c_int, c_int, c_int]),
    'spml_conv_tap_gather_f32': (c_int, [_P, _P, _P, c_int, c_int, c_int, c_int, c_int, _P, _P]),
    'spml_conv_wgrad_pyramid_workspace_bytes': (c_size_t, [c_int, c_int, c_int, c_int, c_int, c_int]),
    'spml_conv_wgrad_pyramid_hl8_f32': (c_int, [_P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, c_int, _P, _P,
                                                c_size_t, _P]),
    'spml_conv_hl8_path_name': (c_char_p, [c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int]),
    'spml_conv_wgrad_path_name': (c_char_p, [c_int, c_int, c_int, c_int, c_int, c_int, c_int]),
    'spml_conv_wgrad_splits': (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, c_int]),
    'spml_bn_stats_ext_f32': (c_int, [_P, c_int64, c_int, _P, _P, _P, _P, _P, c_size_t, _P]),
    'spml_bn_stats_ext_chunks_f32': (c_int, [_P, c_int, c_int, c_int64, c_int, _P, _P, _P, _P, _P]),
    'spml_bn_finalize_f32': (c_int, [_P, _P, c_int, c_double, c_float, c_float, _P, _P, _P, _P]),
    'spml_bn_act_apply_hl8_f32': (c_int, [_P, _P, _P, c_int64, c_int, _P, _P, _P, _P, _P, _P, c_int, _P, _P, _P, _P,
                                          _P]),
    'spml_bn_act_bwd_reduce_ext_f32': (c_int, [_P, _P, _P, _P, c_int64, c_int, _P, _P, _P, _P, _P, _P, c_size_t, _P]),
    'spml_bn_act_bwd_apply_hl8_f32': (c_int, [_P, _P, _P, _P, c_int64, c_int, _P, _P, _P, _P, _P, _P, _P, _P,
                                              c_double, _P, _P, _P, _P, _P, _P]),
    'spml_bn_fwd_hl8_f32': (c_int, [_P, _P, _P, c_int64, c_int, _P, _P, _P, _P, c_float, c_float, c_int, _P, _P, _P, _P,
                                    _P, _P, _P, _P, _P, c_size_t, _P]),
    'spml_bn_bwd_hl8_f32': (c_int, [_P, _P, _P, _P, c_int64, c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P,
                                    c_size_t, _P]),
    'spml_conv_hl8_pyramid_f32': (c_int, [_P, _P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, c_int, _P,
                                          _P]),
    'spml_hl8_weight_transposed_into_f32': (c_int, [_P, c_int, c_int, c_int, _P, _P, c_int, c_int, _P]),
    'spml_absmax_bound_f32': (c_int, [_P, c_int64, _P, c_int, _P]),
    'spml_hl8_weight_set_f32': (c_int, [_P, _P, _P, _P, c_int, _P, _P, _P, _P]),
    'spml_bn_finalize_ranks_f32': (c_int, [_P, c_int, c_int, c_float, c_float, _P, _P, _P, _P, _P, _P]),
    'spml_conv_hl8_affine_f32': (c_int, [_P, _P, _P, _P, _P, _P, c_int, _P, _P, c_int, c_int, c_int, c_int, c_int,
                                         c_int, c_int, _P]),
    'spml_upsample_ce_supported': (c_int, [c_int]),
    'spml_upsample_ce_workspace_bytes': (c_size_t, [c_int, c_int, c_int]),
    'spml_upsample_ce_fwd_f32': (c_int, [_P, _P, c_int, c_int, c_int, c_int, c_int, c_int, c_int64, _P, _P, _P,
                                         c_size_t, _P]),
    'spml_upsample_ce_bwd_f32': (c_int, [_P, _P, _P, c_int, c_int, c_int, c_int, c_int, c_int, c_int64, _P, _P, _P]),
    'spml_upsample_ce_bwd_path_name': (c_char_p, [c_int, c_int, c_int, c_int, c_int, c_int]),
    'spml_bn_stats_f32': (c_int, [_P, c_int64, c_int, _P, _P, _P, c_size_t, _P]),
    'spml_bn_act_apply_f32': (c_int, [_P, _P, c_int64, c_int, _P, _P, _P, _P, c_int, _P, _P]),
    'spml_bn_act_bwd_reduce_f32': (c_int, [_P, _P, _P, c_int64, c_int, _P, _P, _P, _P, _P, c_size_t, _P]),
    'spml_bn_act_bwd_apply_f32': (c_int, [_P, _P, _P, c_int64, c_int, _P, _P, _P, _P, _P, c_double, _P, _P, _P,
                                          _P]),
    'spml_clock_probe': (c_int, [_P, c_int, _P]),
    'spml_maxpool3x3s2_nhwc_f32': (c_int, [_P, c_int, c_int, c_int, c_int, _P, _P]),
    'spml_window_accumulate_f32': (c_int, [_P, c_int, c_int, c_int, _P, _P, c_int, c_int, c_int, c_int,
                                           _P]),
    'spml_unit_hl8_from_nchw_f32': (c_int, [_P, c_int, c_int, c_int, c_int, _P, _P]),
    'spml_class_head_supported': (c_int, [c_int, c_int]),
    'spml_class_head_accumulate_f32': (c_int, [_P, c_int, c_int, c_int, _P, _P, c_int, _P, c_int, c_int, c_int, c_int,
                                               _P]),
    'spml_argmax_channels_i64': (c_int, [_P, c_int, c_int, c_int, c_int, c_int, _P, _P]),
    'spml_iou_counts_i64': (c_int, [_P, _P, c_int64, c_int, _P, _P]),
    'spml_resample_unit_f32': (c_int, [_P, c_int, c_int, c_int, c_int64, c_int64, c_int64, c_int, c_int, c_int, c_int,
                                       c_int, _P, c_int, c_int, _P]),
    'spml_resample_classes_accumulate_f32': (c_int, [_P, c_int, c_int, c_int, c_int64, c_int64, c_int64, c_int, c_int,
                                                     c_int, c_int, c_int, c_int, _P, _P]),
    'spml_cam_finalize_f32': (c_int, [_P, c_int, c_int64, c_int, c_int, _P, c_int, c_float, _P, _P]),
    'spml_upsample_argmax_i64': (c_int, [_P, c_int, c_int, c_int, c_int, c_int, _P, _P]),
    'spml_view_probs_accumulate_f32': (c_int, [_P, c_int, c_int, c_int, _P, _P, c_int, c_int, c_int, c_int, c_int, _P,
                                               _P]),
    'spml_view_votes_workspace_bytes': (c_size_t, [c_int, c_int]),
    'spml_view_votes_accumulate_f32': (c_int, [_P, c_int, c_int, _P, c_int, c_int, c_int, c_int, c_int, c_int, _P, _P,
                                               c_size_t, _P]),
    'spml_segment_majority_workspace_bytes': (c_size_t, [c_int, c_int]),
    'spml_segment_majority_i64': (c_int, [_P, _P, c_int64, c_int, c_int, _P, _P, _P, c_size_t, _P]),
    'spml_segment_majority_path_name': (c_char_p, [c_int64, c_int, c_int]),
    'spml_tag_normalize_workspace_bytes': (c_size_t, [c_int, c_int64]),
    'spml_tag_normalize_argmax_f32': (c_int, [_P, c_int, c_int64, c_int, _P, c_float, _P, _P, _P, _P, c_size_t, _P]),
    'spml_dense_crf_workspace_bytes': (c_size_t, [c_int, c_int, c_int]),
    'spml_dense_crf_prepare_u8': (c_int, [_P, c_int, c_int, c_float, c_float, c_float, _P, c_size_t, _P]),
    'spml_dense_crf_infer_f32': (c_int, [_P, c_int, c_int, c_int, c_int, c_float, c_float, _P, _P, _P, c_size_t, _P]),
    'spml_dense_crf_infer_upsampled_f32': (c_int, [_P, c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_float, _P, _P,
                                                   _P, _P, _P, c_size_t, _P]),
    'spml_dense_crf_votes_workspace_bytes': (c_size_t, [c_int, c_int]),
    'spml_dense_crf_infer_votes_f32': (c_int, [_P, _P, c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_float, _P, _P,
                                               _P, _P, _P, c_size_t, _P, c_size_t, _P]),
    'spml_dense_crf_path_name': (c_char_p, [c_int, c_int, c_int, c_float]),
    'spml_segment_tag_cam_workspace_bytes': (c_size_t, [c_int, c_int]),
    'spml_segment_tag_cam_f32': (c_int, [_P, _P, _P, c_int64, c_float, _P, c_int, c_int, c_int, c_int, c_int, c_int, _P, _P,
                                         _P, _P, c_size_t, _P]),
    'spml_segment_tag_cam_path_name': (c_char_p, [c_int64, c_int, c_int]),
    'spml_augment_params_bytes': (c_size_t, []),
    'spml_augment_path_name': (c_char_p, [_P, c_int64, c_int, c_int]),
    'spml_augment_batch_u8': (c_int, [_P, c_int64, _P, _P, c_int, _P, _P, _P, c_int, c_int, _P, _P, _P, _P]),
    'spml_augment_tags_u8': (c_int, [_P, c_int64, _P, _P, c_int, _P, _P]),
    'spml_view_params_bytes': (c_size_t, []),
    'spml_image_views_path_name': (c_char_p, [_P, c_int, c_int, c_int, c_int64, c_int64, c_int]),
    'spml_image_views_u8': (c_int, [_P, _P, c_int, c_int, _P, _P, _P, _P, c_int, _P, c_int64, _P, c_int64, _P]),
    'spml_label_export_path_name': (c_char_p, [c_int, c_int, c_int, c_int, c_int, c_int]),
    'spml_label_export_u8': (c_int, [_P, c_int, c_int, c_int, c_int, c_int, c_int, _P, _P, _P, _P]),
    'spml_crf_guide_path_name': (c_char_p, [c_int, c_int, c_int, c_int]),
    'spml_crf_guide_u8': (c_int, [_P, c_int, c_int, _P, _P, _P, _P, c_int, c_int, _P, _P]),
    'spml_export_scores_bytes': (c_size_t, [c_int]),
    'spml_label_export_scored_u8': (c_int, [_P, _P, c_int, c_int, c_int, c_int, c_int, c_int, _P, _P, c_int, _P, _P, _P, _P]),
    'spml_score_params_bytes': (c_size_t, []),
    'spml_score_batch_workspace_bytes': (c_size_t, [c_int, c_int]),
    'spml_score_batch_path_name': (c_char_p, [_P, c_int, c_int64, c_int]),
    'spml_score_batch_u8': (c_int, [_P, c_int64, _P, _P, c_int, c_int, _P, _P, c_size_t, _P]),
    'spml_train_summary_workspace_bytes': (c_size_t, [c_int, c_int, c_int, c_int]),
    'spml_pca_path_name': (c_char_p, [c_int, c_int64, c_int64]),
    'spml_pca_moments_f32': (c_int, [_P, c_int, c_int, c_int, c_int, c_int64, c_int64, _P, _P, _P, c_size_t, _P]),
    'spml_pca_project_minmax_f32': (c_int, [_P, c_int, c_int, c_int, c_int, c_int64, c_int64, _P, _P, _P, _P, c_size_t,
                                            _P]),
    'spml_summary_panels_u8': (c_int, [_P, _P, c_int, c_int, c_int, _P, _P, c_int, c_int, _P, c_int, c_int, c_int, _P,
                                       _P]),
    'spml_cam_ingest_path_name': (c_char_p, [c_int, c_int, c_int, c_int]),
    'spml_cam_ingest_f32': (c_int, [_P, _P, c_int, c_int, c_int, c_int, c_int, _P, _P]),
}

EXPORTS = tuple(_SIGNATURES)


class SpmlHipError(RuntimeError):
  pass


ABI_VERSION = 8            # = SPML_ABI_VERSION of include/spml_hip.h (tests/test_cabi_exports.py compares the two)


def lib():
  """Loads libspml_hip.so once; raises if it has not been built."""
  global _lib
  if _lib is None:
    with _lock:
      if _lib is None:
        if not os.path.exists(LIB_PATH):
          raise SpmlHipError(
              'libspml_hip.so not found at %s -- build it with `python -m spml_amd._build` '
              '(there is no CPU fallback for the HIP path)' % LIB_PATH)
        handle = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
          try:
            fn = getattr(handle, name)
          except AttributeError:
            raise SpmlHipError('libspml_hip.so does not export %s (stale build? run '
                               '`python -m spml_amd._build --force`)' % name)
          fn.restype = res
          fn.argtypes = args
        got = handle.spml_abi_version()
        if got != ABI_VERSION:
          raise SpmlHipError('libspml_hip.so has ABI version %d, this wrapper was written against %d (stale build? '
                             'run `python -m spml_amd._build --force`)' % (got, ABI_VERSION))
        exp = handle.spml_build_experiment()
        want = (int(os.environ.get('SPML_CONV_EXP') or 0) & 0xffff) | ((int(os.environ.get('SPML_P64_EXP') or 0) & 0xffff) << 16)
        if exp != want:
          raise SpmlHipError('libspml_hip.so is a profiling build (SPML_CONV_EXP=%d, SPML_P64_EXP=%d: kernels that skip work '
                             'and overwrite outputs) but this process asks for (%d, %d) -- rebuild with '
                             '`python -m spml_amd._build`' % (exp & 0xffff, exp >> 16, want & 0xffff, want >> 16))
        if os.environ.get('SPML_DETERMINISTIC', '0') not in ('', '0'):
          handle.spml_set_deterministic(1)
        _lib = handle
  return _lib


def set_deterministic(on):
  """Deterministic mode of the library (include/spml_hip.h, spml_set_deterministic; also switched on by
  SPML_DETERMINISTIC=1 in the environment when the library is loaded): the segment sums and the prototype gradient
  of the NLL backward are accumulated in 64-bit fixed point instead of through fp32 atomics.  Returns the previous
  setting."""
  return bool(lib().spml_set_deterministic(1 if on else 0))


def deterministic():
  return bool(lib().spml_get_deterministic())


def check(rc, what):
  if rc != 0:
    raise SpmlHipError('%s failed: %s (status %d)' % (
        what, lib().spml_status_string(rc).decode(), rc))


def stream_ptr():
  return c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t, dtype=None, allow_none=False):
  """Device pointer of a contiguous GPU tensor (or NULL)."""
  if t is None:
    if allow_none:
      return c_void_p(0)
    raise SpmlHipError('missing tensor argument')
  if not t.is_cuda:
    raise SpmlHipError('the HIP path needs GPU tensors (got %s); there is no CPU fallback'
                       % t.device)
  if t.device.index != torch.cuda.current_device():
    # kernels are launched on the CURRENT device's current stream with raw pointers
    raise SpmlHipError('tensor lives on %s but the current device is cuda:%d -- wrap the call in '
                       '`torch.cuda.device(tensor.device)`' % (t.device, torch.cuda.current_device()))
  if not t.is_contiguous():
    raise SpmlHipError('tensor must be contiguous')
  if dtype is not None and t.dtype != dtype:
    raise SpmlHipError('expected dtype %s, got %s' % (dtype, t.dtype))
  return c_void_p(t.data_ptr())


def workspace(nbytes, device):
  """A scratch buffer of at least `nbytes` for one library call.  Large sizes are rounded up to 1/8 .. 1/16 of
  themselves: workspaces that follow the prototype / pixel counts of a step drift by a few per cent from step to
  step, and a request a few MB above every cached block made the caching allocator map a new multi-GB segment in the
  middle of a run (config 5: 18 GB in the 7th step, a 480-ms stall; `BENCH_MEM_TRACE=1 python bench.py --recipe
  stress`) -- rounded sizes hit the block of the step before."""
  n = max(int(nbytes), 16)
  if n > (64 << 20):
    g = min(1 << (n.bit_length() - 4), 256 << 20)      # (at most 256 MB of slack: config 5's 18-GB workspace grew by 2 GB)
    n = (n + g - 1) // g * g
  return torch.empty((n,), dtype=torch.uint8, device=device)


# ---------------------------------------------------------------------------
# thin typed wrappers (no autograd here; see spml_amd/ops.py)
# ---------------------------------------------------------------------------

def k1_channels_last(emb, nl):
  """True when K1 can stream `emb` as it is: channels-last storage and a channel count the row-wise
  kernels take (no NHWC -> NCHW copy in front of K1, none behind its backward)."""
  return (emb.dim() == 4 and emb.dtype == torch.float32 and not emb.is_contiguous() and
          emb.is_contiguous(memory_format=torch.channels_last) and
          bool(lib().spml_normalize_concat_local_nhwc_supported(int(emb.shape[1]), int(nl))))


def normalize_concat_loc(emb, loc=None, row_map=None, num_rows=None, want_emb=True,
                         want_loc=True):
  n, c, h, w = emb.shape
  nl = 2 if loc is None else int(loc.shape[-1])       # local-feature channels ((y, x) = 2)
  rows = n * h * w if num_rows is None else int(num_rows)
  out_emb = torch.empty((rows, c), dtype=torch.float32, device=emb.device) if want_emb else None
  out_loc = torch.empty((rows, c + nl), dtype=torch.float32, device=emb.device) if want_loc else None
  if k1_channels_last(emb, nl):
    check(lib().spml_normalize_concat_local_nhwc_f32(
        _ptr_any(emb), n, c, h, w, ptr(loc, torch.float32, True), nl,
        ptr(row_map, torch.int64, True), ptr(out_emb, None, True), ptr(out_loc, None, True),
        stream_ptr()), 'spml_normalize_concat_local_nhwc_f32')
    return out_emb, out_loc
  check(lib().spml_normalize_concat_local_f32(
      ptr(emb, torch.float32), n, c, h, w, ptr(loc, torch.float32, True), nl,
      ptr(row_map, torch.int64, True), ptr(out_emb, None, True), ptr(out_loc, None, True),
      stream_ptr()), 'spml_normalize_concat_local_f32')
  return out_emb, out_loc


def normalize_concat_loc_bwd(emb, loc, row_map, d_out_emb, d_out_loc):
  n, c, h, w = emb.shape
  nl = 2 if loc is None else int(loc.shape[-1])
  d_emb = torch.empty_like(emb)                        # (keeps the memory format of emb)
  if k1_channels_last(emb, nl):
    check(lib().spml_normalize_concat_local_nhwc_bwd_f32(
        _ptr_any(emb), n, c, h, w, ptr(loc, torch.float32, True), nl,
        ptr(row_map, torch.int64, True), ptr(d_out_emb, torch.float32, True),
        ptr(d_out_loc, torch.float32, True), _ptr_any(d_emb), stream_ptr()),
          'spml_normalize_concat_local_nhwc_bwd_f32')
    return d_emb
  check(lib().spml_normalize_concat_local_bwd_f32(
      ptr(emb, torch.float32), n, c, h, w, ptr(loc, torch.float32, True), nl,
      ptr(row_map, torch.int64, True), ptr(d_out_emb, torch.float32, True),
      ptr(d_out_loc, torch.float32, True), ptr(d_emb), stream_ptr()),
        'spml_normalize_concat_local_bwd_f32')
  return d_emb


def normalize_rows(x):
  d = x.shape[-1]
  x2 = x.reshape(-1, d)
  y = torch.empty_like(x2)
  check(lib().spml_normalize_rows_f32(ptr(x2, torch.float32), x2.shape[0], d, ptr(y),
                                      stream_ptr()), 'spml_normalize_rows_f32')
  return y.view(x.shape)


def normalize_rows_bwd(x, dy):
  d = x.shape[-1]
  x2, g2 = x.reshape(-1, d), dy.reshape(-1, d).contiguous()
  dx = torch.empty_like(x2)
  check(lib().spml_normalize_rows_bwd_f32(ptr(x2, torch.float32), ptr(g2, torch.float32),
                                          x2.shape[0], d, ptr(dx), stream_ptr()),
        'spml_normalize_rows_bwd_f32')
  return dx.view(x.shape)


def kmeans_init_grid(h, w, ky, kx, device):
  out = torch.empty((h, w), dtype=torch.int64, device=device)
  check(lib().spml_kmeans_init_grid_i64(h, w, ky, kx, ptr(out), stream_ptr()),
        'spml_kmeans_init_grid_i64')
  return out


_last_kmeans = None        # arguments of this thread's last k-means call (for kmeans_last_path)


def relabel_unique(keys, with_uniq=True, padded=False):
  """-> (uniq, inv [P], count [1] device tensor).  with_uniq: `uniq` = the U sorted distinct keys (the
  count is read on the host: one sync); padded: `uniq` has P entries, the sorted distinct keys followed
  by INT64_MAX (still sorted; no sync); neither: `uniq` is None and nothing synchronises.
  Keys: any int64 except INT64_MIN (the empty-slot sentinel of the hash set; the callers build keys from
  non-negative labels).  Cost ~ P + U^2 / 2048 * 11 compares: meant for U << P (segments, not pixels)."""
  keys = keys.reshape(-1)
  if keys.dtype != torch.int64 or not keys.is_contiguous():
    keys = keys.long().contiguous()
  p = keys.shape[0]
  inv = torch.empty((p,), dtype=torch.int64, device=keys.device)
  count = torch.empty((1,), dtype=torch.int64, device=keys.device)
  if padded:
    uniq = torch.full((p,), torch.iinfo(torch.int64).max, dtype=torch.int64, device=keys.device)
  else:
    uniq = torch.empty((p if with_uniq else 0,), dtype=torch.int64, device=keys.device)
  ws = workspace(lib().spml_relabel_unique_workspace_bytes(p), keys.device)
  check(lib().spml_relabel_unique_i64(ptr(keys, torch.int64, p == 0), p, ptr(inv, allow_none=p == 0),
                                      ptr(uniq, allow_none=uniq.numel() == 0), uniq.numel(), ptr(count), ptr(ws),
                                      ws.numel(), stream_ptr()), 'spml_relabel_unique_i64')
  if padded:
    return uniq, inv, count
  if not with_uniq:
    return None, inv, count
  return uniq[:int(count.item())], inv, count


def _note_kmeans(p, d, k, n_img, max_seg_len, iterations, given, flags):
  global _last_kmeans
  _last_kmeans = (int(p), int(d), int(k), int(n_img), int(max_seg_len), int(iterations), int(given),
                  int(flags))


def kmeans_path_name(p, d, k, n_img, max_seg_len, iterations, given_centroids=False, flags=0):
  """Code path a k-means call with these arguments takes (a pure function of the library)."""
  return lib().spml_kmeans_path_name(int(p), int(d), int(k), int(n_img), int(max_seg_len),
                                     int(iterations), int(bool(given_centroids)), int(flags)).decode()


def kmeans_last_path():
  """Path name of the last k-means call made through this module (Python-side bookkeeping
  over spml_kmeans_path_name; the library keeps no state)."""
  return 'none' if _last_kmeans is None else lib().spml_kmeans_path_name(*_last_kmeans).decode()


def kmeans_run(x, seg_offsets, max_seg_len, k, labels_init, iterations, want_centroids=False,
               flags=0):
  p, d = x.shape
  n_img = seg_offsets.shape[0] - 1
  labels = torch.empty((p,), dtype=torch.int64, device=x.device)
  cent = (torch.zeros((n_img, k, d), dtype=torch.float32, device=x.device)
          if want_centroids else None)
  nbytes = lib().spml_kmeans_workspace_bytes(p, d, k, n_img, max_seg_len)
  ws = workspace(nbytes, x.device)
  check(lib().spml_kmeans_run_f32(
      ptr(x, torch.float32), p, d, ptr(seg_offsets, torch.int64), n_img, int(max_seg_len), k,
      ptr(labels_init, torch.int64), int(iterations), ptr(labels), ptr(cent, None, True),
      int(flags), ptr(ws), ws.numel(), stream_ptr()), 'spml_kmeans_run_f32')
  _note_kmeans(p, d, k, n_img, max_seg_len, iterations, 0, flags)
  return (labels, cent) if want_centroids else labels


def kmeans_run_profiled(x, seg_offsets, max_seg_len, k, labels_init, iterations, flags=0):
  """-> (labels, durations_us [iterations + 1]): every pass kernel's duration from the
  per-workgroup device time stamps (max end - min start, 100-MHz s_memrealtime)."""
  import ctypes
  p, d = x.shape
  n_img = seg_offsets.shape[0] - 1
  n_pass, wgs = ctypes.c_int(0), ctypes.c_int(0)
  check(lib().spml_kmeans_profile_layout(p, d, k, n_img, int(max_seg_len), int(iterations),
                                         ctypes.byref(n_pass), ctypes.byref(wgs)),
        'spml_kmeans_profile_layout')
  clocks = torch.zeros((n_pass.value, wgs.value, 2), dtype=torch.int64, device=x.device)
  labels = torch.empty((p,), dtype=torch.int64, device=x.device)
  ws = workspace(lib().spml_kmeans_workspace_bytes(p, d, k, n_img, max_seg_len), x.device)
  check(lib().spml_kmeans_run_profiled_f32(
      ptr(x, torch.float32), p, d, ptr(seg_offsets, torch.int64), n_img, int(max_seg_len), k,
      ptr(labels_init, torch.int64), int(iterations), ptr(labels), int(flags), ptr(ws), ws.numel(),
      ptr(clocks), clocks.numel(), stream_ptr()), 'spml_kmeans_run_profiled_f32')
  _note_kmeans(p, d, k, n_img, max_seg_len, iterations, 0, flags)
  c = clocks.cpu()
  # (passes may run fewer workgroups than the layout's maximum: their stamps stay zero)
  start = torch.where(c[:, :, 0] == 0, torch.full_like(c[:, :, 0], torch.iinfo(torch.int64).max), c[:, :, 0])
  dur = (c[:, :, 1].max(dim=1).values - start.min(dim=1).values).double() * 0.01
  return labels, dur


def kmeans_assign(x, seg_offsets, max_seg_len, centroids, flags=0):
  p, d = x.shape
  n_img = seg_offsets.shape[0] - 1
  k = centroids.shape[-2]
  labels = torch.empty((p,), dtype=torch.int64, device=x.device)
  nbytes = lib().spml_kmeans_workspace_bytes(p, d, k, n_img, max_seg_len)
  ws = workspace(nbytes, x.device)
  check(lib().spml_kmeans_assign_f32(
      ptr(x, torch.float32), p, d, ptr(seg_offsets, torch.int64), n_img, int(max_seg_len), k,
      ptr(centroids, torch.float32), ptr(labels), int(flags), ptr(ws), ws.numel(),
      stream_ptr()), 'spml_kmeans_assign_f32')
  _note_kmeans(p, d, k, n_img, max_seg_len, 1, 1, flags)
  return labels


def kmeans_workspace(x, seg_offsets, max_seg_len, k):
  p, d = x.shape
  return workspace(lib().spml_kmeans_workspace_bytes(p, d, k, seg_offsets.shape[0] - 1, max_seg_len),
                   x.device)


def kmeans_preconvert(x, seg_offsets, max_seg_len, k, ws):
  """X -> split-f16 tiles inside `ws` (for kmeans_fused_pass(..., preconverted=True))."""
  p, d = x.shape
  check(lib().spml_kmeans_preconvert_f32(
      ptr(x, torch.float32), p, d, ptr(seg_offsets, torch.int64), seg_offsets.shape[0] - 1,
      int(max_seg_len), int(k), ptr(ws), ws.numel(), stream_ptr()), 'spml_kmeans_preconvert_f32')


def kmeans_fused_pass(x, seg_offsets, max_seg_len, centroids, ws=None, preconverted=False, flags=0,
                      out=None):
  """One fused pass: (labels [P] int64, raw sums [n_img,K,D] of X by the new labels)."""
  p, d = x.shape
  n_img = seg_offsets.shape[0] - 1
  k = centroids.shape[-2]
  if ws is None:
    ws = kmeans_workspace(x, seg_offsets, max_seg_len, k)
  if out is None:
    out = (torch.empty((p,), dtype=torch.int64, device=x.device),
           torch.empty((n_img, k, d), dtype=torch.float32, device=x.device))
  labels, sums = out
  flags = int(flags) | (32 if preconverted else 0)
  check(lib().spml_kmeans_fused_pass_f32(
      ptr(x, torch.float32), p, d, ptr(seg_offsets, torch.int64), n_img, int(max_seg_len), k,
      ptr(centroids, torch.float32), ptr(labels, torch.int64), ptr(sums, torch.float32), flags,
      ptr(ws), ws.numel(), stream_ptr()), 'spml_kmeans_fused_pass_f32')
  _note_kmeans(p, d, k, n_img, max_seg_len, 1, 1, flags)
  return labels, sums


def clock_probe(device, spin_us, stream):
  """Launches the clock probe on `stream` (a torch.cuda.Stream); returns the device tensor [cycles, 100-MHz ticks]
  (read it after synchronising): shader clock in MHz = 100 * cycles / ticks."""
  out = torch.zeros((2,), dtype=torch.int64, device=device)
  # the probe starts where the current stream stands now (behind the zero fill of `out` and everything queued in front
  # of it), not at once: it measures the clock of what the caller launches NEXT on the current stream
  stream.wait_stream(torch.cuda.current_stream(device))
  check(lib().spml_clock_probe(ptr(out), int(spin_us), c_void_p(stream.cuda_stream)), 'spml_clock_probe')
  return out


def maxpool3x3s2_nhwc(x):
  """nn.MaxPool2d(3, 2, 1) of a channels-last fp32 map (forward only) -> channels-last map."""
  n, c, h, w = x.shape
  oh, ow = (h - 1) // 2 + 1, (w - 1) // 2 + 1
  y = torch.empty((n, c, oh, ow), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
  check(lib().spml_maxpool3x3s2_nhwc_f32(_ptr_any(x), n, h, w, c, _ptr_any(y), stream_ptr()), 'spml_maxpool3x3s2_nhwc_f32')
  return y


def segment_sum_normalize(x, ids, m):
  p, d = x.shape
  sums = torch.empty((m, d), dtype=torch.float32, device=x.device)
  protos = torch.empty((m, d), dtype=torch.float32, device=x.device)
  if deterministic():
    nbytes = lib().spml_segment_sum_det_workspace_bytes(int(m), d)
    ws = workspace(nbytes, x.device)
    check(lib().spml_segment_sum_normalize_det_f32(ptr(x, torch.float32), ptr(ids, torch.int64), p, d, int(m),
                                                   ptr(sums), ptr(protos), ptr(ws), ws.numel(), stream_ptr()),
          'spml_segment_sum_normalize_det_f32')
    return protos, sums
  check(lib().spml_segment_sum_normalize_f32(ptr(x, torch.float32), ptr(ids, torch.int64), p, d,
                                             int(m), ptr(sums), ptr(protos), stream_ptr()),
        'spml_segment_sum_normalize_f32')
  return protos, sums


def segment_sum_normalize_bwd(d_protos, sums, ids, p, accumulate=0, dx=None):
  """-> dx [p, D].  accumulate != 0: the gradient is ADDED into the given `dx` (which the call returns)."""
  m, d = sums.shape
  scratch = torch.empty_like(sums)
  if accumulate:
    if dx is None or tuple(dx.shape) != (p, d):
      raise SpmlHipError('accumulate needs a dx of shape (%d, %d) to add into' % (p, d))
  else:
    dx = torch.empty((p, d), dtype=torch.float32, device=sums.device)
  check(lib().spml_segment_sum_normalize_bwd_f32(
      ptr(d_protos, torch.float32), ptr(sums, torch.float32), ptr(ids, torch.int64), p, d, m,
      ptr(scratch), ptr(dx, torch.float32), 1 if accumulate else 0, stream_ptr()), 'spml_segment_sum_normalize_bwd_f32')
  return dx


def segsort_nll_fwd(emb, own, px_code, protos, pr_code, kappa, mode):
  p, d = emb.shape
  m = protos.shape[0]
  nll = torch.empty((p,), dtype=torch.float32, device=emb.device)
  stats = torch.empty((p, 4), dtype=torch.float32, device=emb.device)
  ws = workspace(lib().spml_segsort_nll_workspace_bytes(p, m, d), emb.device)
  check(lib().spml_segsort_nll_fwd_f32(
      ptr(emb, torch.float32), ptr(own, torch.int64), ptr(px_code, torch.int64), p,
      ptr(protos, torch.float32), ptr(pr_code, torch.int64), m, d, float(kappa), int(mode),
      ptr(nll), ptr(stats), ptr(ws), ws.numel(), stream_ptr()), 'spml_segsort_nll_fwd_f32')
  return nll, stats


def segsort_nll_bwd(emb, own, px_code, protos, pr_code, kappa, mode, stats, d_nll, m_grad=-1):
  p, d = emb.shape
  m = protos.shape[0]
  d_emb = torch.empty_like(emb)
  d_protos = torch.zeros_like(protos)
  ws = workspace(lib().spml_segsort_nll_workspace_bytes(p, m, d), emb.device)
  check(lib().spml_segsort_nll_bwd_f32(
      ptr(emb, torch.float32), ptr(own, torch.int64), ptr(px_code, torch.int64), p,
      ptr(protos, torch.float32), ptr(pr_code, torch.int64), m, d, float(kappa), int(mode),
      ptr(stats, torch.float32), ptr(d_nll, torch.float32), ptr(d_emb), ptr(d_protos),
      int(m_grad), ptr(ws), ws.numel(), stream_ptr()), 'spml_segsort_nll_bwd_f32')
  return d_emb, d_protos


def segsort_nll_path_name(p, m, d, mode, backward=False, m_grad=-1):
  """What segsort_nll_fwd / segsort_nll_bwd launches for these sizes under the current environment and deterministic
  mode (include/spml_hip.h, spml_segsort_nll_path_name: the library's own predicates, no GPU call)."""
  buf = ctypes.create_string_buffer(160)
  check(lib().spml_segsort_nll_path_name(int(p), int(m), int(d), int(mode), 1 if backward else 0, int(m_grad),
                                         buf, len(buf)), 'spml_segsort_nll_path_name')
  return buf.value.decode()


def segsort_nll_batched_supported(d, mode):
  """True when the batched NLL entry points take this embedding width and mode (include/spml_hip.h)."""
  return bool(lib().spml_segsort_nll_batched_supported(int(d), int(mode)))


def _host_offsets(sizes):
  """Host prefix array [n + 1] of a list of sizes (the library reads it during the call only)."""
  off = (c_int64 * (len(sizes) + 1))()
  for i, v in enumerate(sizes):
    off[i + 1] = off[i] + int(v)
  return off


def _nll_batched_workspace(p_off, m_off, n, d, device):
  nbytes = lib().spml_segsort_nll_batched_workspace_bytes(n, p_off, m_off, d)
  if nbytes == 0 and n > 0:
    raise SpmlHipError('spml_segsort_nll_batched_workspace_bytes refused the sizes (D = %d)' % d)
  return workspace(nbytes, device)


def segsort_nll_batched_fwd(emb, own_abs, px_code, p_sizes, protos, pr_code, m_sizes, kappa, mode):
  """N problems in one call: problem i owns p_sizes[i] consecutive pixel rows and m_sizes[i] consecutive
  prototype rows; own_abs indexes the concatenated prototypes."""
  p, d = emb.shape
  n = len(p_sizes)
  p_off, m_off = _host_offsets(p_sizes), _host_offsets(m_sizes)
  if len(m_sizes) != n or p_off[n] != p or m_off[n] != protos.shape[0]:
    raise SpmlHipError('the problem sizes do not add up to the rows given')
  nll = torch.empty((p,), dtype=torch.float32, device=emb.device)
  stats = torch.empty((p, 4), dtype=torch.float32, device=emb.device)
  ws = _nll_batched_workspace(p_off, m_off, n, d, emb.device)
  check(lib().spml_segsort_nll_batched_fwd_f32(
      ptr(emb, torch.float32), ptr(own_abs, torch.int64), ptr(px_code, torch.int64), p_off,
      ptr(protos, torch.float32), ptr(pr_code, torch.int64), m_off, n, d, float(kappa), int(mode),
      ptr(nll), ptr(stats), ptr(ws), ws.numel(), stream_ptr()), 'spml_segsort_nll_batched_fwd_f32')
  return nll, stats


def segsort_nll_batched_bwd(emb, own_abs, px_code, p_sizes, protos, pr_code, m_sizes, kappa, mode, stats, d_nll):
  p, d = emb.shape
  n = len(p_sizes)
  p_off, m_off = _host_offsets(p_sizes), _host_offsets(m_sizes)
  if len(m_sizes) != n or p_off[n] != p or m_off[n] != protos.shape[0] or \
      stats.shape[0] != p or d_nll.shape[0] != p:
    raise SpmlHipError('the problem sizes do not add up to the rows given')
  d_emb = torch.empty_like(emb)
  d_protos = torch.zeros_like(protos)
  ws = _nll_batched_workspace(p_off, m_off, n, d, emb.device)
  check(lib().spml_segsort_nll_batched_bwd_f32(
      ptr(emb, torch.float32), ptr(own_abs, torch.int64), ptr(px_code, torch.int64), p_off,
      ptr(protos, torch.float32), ptr(pr_code, torch.int64), m_off, n, d, float(kappa), int(mode),
      ptr(stats, torch.float32), ptr(d_nll, torch.float32), ptr(d_emb), ptr(d_protos),
      ptr(ws), ws.numel(), stream_ptr()), 'spml_segsort_nll_batched_bwd_f32')
  return d_emb, d_protos


def topk_affinity(q, protos, k, q_group=None, pr_group=None, pr_valid=None, masked_value=-2.0):
  nq, d = q.shape
  m = protos.shape[0]
  idx = torch.empty((nq, k), dtype=torch.int64, device=q.device)
  val = torch.empty((nq, k), dtype=torch.float32, device=q.device)
  ws = workspace(lib().spml_topk_workspace_bytes(nq, m, d, k), q.device)
  check(lib().spml_topk_affinity_f32(
      ptr(q, torch.float32), nq, ptr(protos, torch.float32), m, d, int(k),
      ptr(q_group, torch.int64, True), ptr(pr_group, torch.int64, True),
      ptr(pr_valid, torch.uint8, True), float(masked_value), ptr(idx), ptr(val), ptr(ws),
      ws.numel(), stream_ptr()), 'spml_topk_affinity_f32')
  return idx, val


def window_accumulate(patch, acc, counts, sh, sw):
  """acc[:, sh:sh+h, sw:sw+w] += patch / |patch|_channels ; counts[window] += 1 (in place)."""
  c, h, w = patch.shape
  big_c, big_h, big_w = acc.shape
  if big_c != c or tuple(counts.shape) != (big_h, big_w):
    raise SpmlHipError('window_accumulate: shape mismatch')
  check(lib().spml_window_accumulate_f32(
      ptr(patch, torch.float32), c, h, w, ptr(acc, torch.float32), ptr(counts, torch.float32),
      big_h, big_w, int(sh), int(sw), stream_ptr()), 'spml_window_accumulate_f32')


# ---------------------------------------------------------------------------
# full-resolution softmax inference (csrc/softmax_head.hip)
def unit_hl8_from_nchw(x):
  """x fp32 [n, C, h, w] (NCHW, contiguous) -> Hl8 [n*h*w, C] of x / |x| over the channels; its bound is a device
  1.0 (a unit row: the scale is fixed, no abs-max pass)."""
  n, c, h, w = x.shape
  out = torch.empty((n * h * w * c * 4,), dtype=torch.uint8, device=x.device)
  check(lib().spml_unit_hl8_from_nchw_f32(ptr(x, torch.float32), n, c, h, w, ptr(out), stream_ptr()),
        'spml_unit_hl8_from_nchw_f32')
  return Hl8(out, torch.ones((1,), dtype=torch.float32, device=x.device), n * h * w, c)


def class_head_supported(ch, ncls):
  return bool(lib().spml_class_head_supported(int(ch), int(ncls)))


def class_head_accumulate(hidden, weight, bias, canvas, sh, sw, h, w):
  """canvas[:, sh:sh+h, sw:sw+w] += hidden @ weight.T + bias (in place).  hidden: fp32, h*w*Ch values stored
  channels-last (any shape); weight [ncls, Ch]; canvas [ncls, Hp, Wp]."""
  ncls, ch = weight.shape
  if hidden.numel() != h * w * ch or canvas.dim() != 3 or canvas.shape[0] != ncls or bias.numel() != ncls:
    raise SpmlHipError('class_head_accumulate: shape mismatch')
  check(lib().spml_class_head_accumulate_f32(
      _ptr_any(hidden), ch, int(h), int(w), ptr(weight, torch.float32), ptr(bias, torch.float32), ncls,
      ptr(canvas, torch.float32), canvas.shape[1], canvas.shape[2], int(sh), int(sw), stream_ptr()),
        'spml_class_head_accumulate_f32')


def argmax_channels(canvas, h, w):
  """canvas fp32 [ncls, Hp, Wp] -> int64 [h, w]: arg-max over the classes of the top-left region."""
  ncls, hp, wp = canvas.shape
  out = torch.empty((h, w), dtype=torch.int64, device=canvas.device)
  check(lib().spml_argmax_channels_i64(ptr(canvas, torch.float32), ncls, hp, wp, int(h), int(w), ptr(out),
                                       stream_ptr()), 'spml_argmax_channels_i64')
  return out


def iou_counts(pred, target, ncls, counts=None):
  """counts int64 [3, ncls] += (TP+FN, TP+FP, TP) of two int64 label maps (a fresh zero tensor when None)."""
  if pred.numel() != target.numel():
    raise SpmlHipError('iou_counts: pred and target differ in size')
  if counts is None:
    counts = torch.zeros((3, ncls), dtype=torch.int64, device=pred.device)
  elif tuple(counts.shape) != (3, ncls):
    raise SpmlHipError('iou_counts: counts must be [3, num_classes]')
  check(lib().spml_iou_counts_i64(ptr(pred, torch.int64), ptr(target, torch.int64), pred.numel(), int(ncls),
                                  ptr(counts, torch.int64), stream_ptr()), 'spml_iou_counts_i64')
  return counts


# ---------------------------------------------------------------------------
# pseudo-label generation (csrc/pseudo_label.hip)
COMBINE_MODES = {'prob_mean': 0, 'logit_mean': 1}      # SPML_COMBINE_* of include/spml_hip.h


def _combine(combine):
  if combine not in COMBINE_MODES:
    raise SpmlHipError("combine must be 'prob_mean' or 'logit_mean' (got %r)" % (combine,))
  return COMBINE_MODES[combine]


def _view_args(x, crop_hw, out_hw, what):
  """(C, Hp, Wp, strides..., rh, rw, oh, ow) of a network output [C, Hp, Wp] read through its strides."""
  if x.dim() != 3:
    raise SpmlHipError('%s: expected a [C, Hp, Wp] tensor' % what)
  c, hp, wp = x.shape
  (rh, rw), (oh, ow) = crop_hw, out_hw
  if not (0 < rh <= hp and 0 < rw <= wp and oh > 0 and ow > 0):
    raise SpmlHipError('%s: crop %r / output %r do not fit a %d x %d plane' % (what, crop_hw, out_hw, hp, wp))
  sc, sy, sx = x.stride()
  return c, hp, wp, sc, sy, sx, int(rh), int(rw), int(oh), int(ow)


def resample_unit(emb, crop_hw, flip, out_hw, out, b):
  """out[b] = unit-norm columns of `emb` [C, Hp, Wp] (fp32, any positive strides: NCHW or channels-last, no copy)
  cropped to its top-left `crop_hw`, flipped back when `flip`, bilinearly resampled to `out_hw`.  out: fp32
  [B, C, oh*ow] (contiguous), the operand of `affinity_transition`."""
  c, hp, wp, sc, sy, sx, rh, rw, oh, ow = _view_args(emb, crop_hw, out_hw, 'resample_unit')
  if out.dim() != 3 or out.shape[1] != c or out.shape[2] != oh * ow or not 0 <= b < out.shape[0]:
    raise SpmlHipError('resample_unit: out must be [B, %d, %d] with b < B' % (c, oh * ow))
  check(lib().spml_resample_unit_f32(_ptr_any(emb), c, hp, wp, sc, sy, sx, rh, rw, int(bool(flip)), oh, ow,
                                     ptr(out, torch.float32), out.shape[0], int(b), stream_ptr()),
        'spml_resample_unit_f32')
  return out


def resample_classes_accumulate(logit, crop_hw, flip, out_hw, acc, combine='prob_mean'):
  """acc += the view `logit` [ncls, Hp, Wp] (fp32, any positive strides) cropped, un-flipped, resampled to `out_hw` and
  -- with combine='prob_mean' -- soft-maxed over the classes; 'logit_mean' adds the resampled logits.  acc: fp32
  [ncls, oh*ow] (or [ncls, oh, ow]), contiguous, updated in place."""
  ncls, hp, wp, sc, sy, sx, rh, rw, oh, ow = _view_args(logit, crop_hw, out_hw, 'resample_classes_accumulate')
  if acc.shape[0] != ncls or acc.numel() != ncls * oh * ow:
    raise SpmlHipError('resample_classes_accumulate: acc must hold [%d, %d] values' % (ncls, oh * ow))
  check(lib().spml_resample_classes_accumulate_f32(_ptr_any(logit), ncls, hp, wp, sc, sy, sx, rh, rw, int(bool(flip)),
                                                   oh, ow, _combine(combine), ptr(acc, torch.float32), stream_ptr()),
        'spml_resample_classes_accumulate_f32')
  return acc


def cam_finalize(acc, num_views, label_tags, combine='prob_mean', background_threshold=None):
  """Summed views `acc` [ncls, ...] -> class activation maps of the same shape: mean over the views, softmax over the
  classes for 'logit_mean', every class divided by its maximum, untagged classes 0, class 0 = `background_threshold`
  when given.  label_tags: bool (or uint8) [ncls] on the device."""
  ncls = acc.shape[0]
  if label_tags.numel() != ncls or label_tags.dtype not in (torch.bool, torch.uint8):
    raise SpmlHipError('cam_finalize: label_tags must be a bool [%d] tensor' % ncls)
  if int(num_views) < 1:
    raise SpmlHipError('cam_finalize: no views')
  cam = torch.empty_like(acc)
  tags = label_tags.view(torch.uint8) if label_tags.dtype == torch.bool else label_tags
  check(lib().spml_cam_finalize_f32(ptr(acc, torch.float32), ncls, acc.numel() // ncls, int(num_views),
                                    _combine(combine), ptr(tags, torch.uint8), int(background_threshold is not None),
                                    float(background_threshold or 0.0), ptr(cam), stream_ptr()),
        'spml_cam_finalize_f32')
  return cam


def upsample_argmax(cam, h, w):
  """cam fp32 [ncls, oh, ow] -> int64 [h, w]: arg-max over the classes of the bilinearly up-sampled maps (which are
  never materialised)."""
  if cam.dim() != 3:
    raise SpmlHipError('upsample_argmax: expected [ncls, oh, ow]')
  ncls, oh, ow = cam.shape
  out = torch.empty((int(h), int(w)), dtype=torch.int64, device=cam.device)
  check(lib().spml_upsample_argmax_i64(ptr(cam, torch.float32), ncls, oh, ow, int(h), int(w), ptr(out), stream_ptr()),
        'spml_upsample_argmax_i64')
  return out


# ---------------------------------------------------------------------------
# multi-scale + flip softmax inference (csrc/msc_inference.hip)
def view_probs_accumulate(canvas, cnt_y, cnt_x, crop_hw, flip, acc):
  """acc += softmax over the classes of one view: `canvas` [ncls, Hp, Wp] (the summed window logits) divided by the
  overlap counts `cnt_y[:, None] * cnt_x[None, :]`, cropped to its top-left `crop_hw`, bilinearly resampled to the
  `[h, w]` of `acc` [ncls, h, w] and -- when `flip` -- mirrored AFTER the softmax (inference_softmax_msc.py:135-147).
  All four tensors fp32, contiguous, on the GPU; acc is updated in place and returned."""
  if canvas.dim() != 3 or acc.dim() != 3 or acc.shape[0] != canvas.shape[0]:
    raise SpmlHipError('view_probs_accumulate: canvas must be [ncls, Hp, Wp] and acc [ncls, h, w]')
  ncls, hp, wp = canvas.shape
  rh, rw = int(crop_hw[0]), int(crop_hw[1])
  if not (0 < rh <= hp and 0 < rw <= wp):
    raise SpmlHipError('view_probs_accumulate: crop %r does not fit a %d x %d plane' % (tuple(crop_hw), hp, wp))
  if tuple(cnt_y.shape) != (hp,) or tuple(cnt_x.shape) != (wp,):
    raise SpmlHipError('view_probs_accumulate: cnt_y must be [%d] and cnt_x [%d]' % (hp, wp))
  check(lib().spml_view_probs_accumulate_f32(
      ptr(canvas, torch.float32), ncls, hp, wp, ptr(cnt_y, torch.float32), ptr(cnt_x, torch.float32), rh, rw,
      int(bool(flip)), acc.shape[1], acc.shape[2], ptr(acc, torch.float32), stream_ptr()),
        'spml_view_probs_accumulate_f32')
  return acc


# ---------------------------------------------------------------------------
# multi-scale + flip kNN inference (csrc/knn_msc.hip)
MAX_VIEW_VOTES_CLASSES = 64            # the limits of spml_view_votes_accumulate_f32 (include/spml_hip.h)
MAX_VIEW_VOTES_SEGMENTS = 4096


def view_votes_accumulate(clu, crop_hw, topk, ncls, flip, acc):
  """acc += the class votes of one view: `clu` int64 `[rh * rw]` (or `[rh, rw]`), the dense segment id of every pixel of
  the un-padded view; `topk` int64 `[m, k]`, the labels retrieved per segment; votes[s][c] = the share of `topk[s]` equal
  to c, gathered by `clu`, bilinearly resampled from `crop_hw` to the `[h, w]` of `acc` `[ncls, h, w]` (fp32) and -- when
  `flip` -- mirrored afterwards (inference_msc.py:223-234, the sum of :237-239).  All tensors contiguous, on the GPU; acc
  is updated in place and returned."""
  rh, rw = int(crop_hw[0]), int(crop_hw[1])
  if rh < 1 or rw < 1 or clu.numel() != rh * rw:
    raise SpmlHipError('view_votes_accumulate: clu must hold %d x %d segment ids' % (rh, rw))
  if topk.dim() != 2 or acc.dim() != 3 or acc.shape[0] != int(ncls):
    raise SpmlHipError('view_votes_accumulate: topk must be [m, k] and acc [%d, h, w]' % int(ncls))
  m, k = topk.shape
  nbytes = lib().spml_view_votes_workspace_bytes(int(m), int(ncls))
  if nbytes == 0:
    raise SpmlHipError('view_votes_accumulate: %d segments x %d classes are outside the kernel (at most %d x %d)'
                       % (m, ncls, MAX_VIEW_VOTES_SEGMENTS, MAX_VIEW_VOTES_CLASSES))
  ws = workspace(nbytes, acc.device)
  check(lib().spml_view_votes_accumulate_f32(
      ptr(clu, torch.int64), rh, rw, ptr(topk, torch.int64), int(m), int(k), int(ncls), int(bool(flip)),
      acc.shape[1], acc.shape[2], ptr(acc, torch.float32), ptr(ws), ws.numel(), stream_ptr()),
        'spml_view_votes_accumulate_f32')
  return acc


# ---------------------------------------------------------------------------
# memory-bank generation: majority label per segment (csrc/segment_majority.hip)
MAX_MAJORITY_SEGMENTS = 4096           # the limits of spml_segment_majority_i64 (include/spml_hip.h)
MAX_MAJORITY_CLASSES = 256


def segment_majority_path_name(p, m, ncls):
  """Count kernel a call with these sizes takes (a pure function of the library): 'lds_table' or 'global_table'."""
  return lib().spml_segment_majority_path_name(int(p), int(m), int(ncls)).decode()


def segment_majority(clu, sem, m, ncls, want_hist=False):
  """major int64 `[m]`: the most frequent class of `sem` among the pixels of every segment of `clu` (both int64, one
  entry per pixel, any shape; made contiguous here), ties to the lowest class, 0 for a segment without a counted pixel
  (segsort/common.py:221-267 without the list of agreeing pixels).  An id outside `[0, m)` or a class outside
  `[0, ncls)` counts nowhere.  No host read.  want_hist: -> (major, hist int64 `[m, ncls]`), the counts."""
  clu, sem = clu.reshape(-1), sem.reshape(-1)
  if clu.numel() != sem.numel():
    raise SpmlHipError('segment_majority: %d segment ids for %d labels' % (clu.numel(), sem.numel()))
  for name, t in (('clu', clu), ('sem', sem)):
    if t.dtype != torch.int64:
      raise SpmlHipError('segment_majority: %s must be int64 (got %s)' % (name, t.dtype))
  clu, sem = clu.contiguous(), sem.contiguous()
  p, m, ncls = clu.numel(), int(m), int(ncls)
  if m < 1 or ncls < 1:
    raise SpmlHipError('segment_majority: needs at least one segment and one class (got %d, %d)' % (m, ncls))
  ptr(clu), ptr(sem)                                         # (CPU tensors are refused before anything is allocated)
  major = torch.empty((m,), dtype=torch.int64, device=clu.device)
  hist = torch.empty((m, ncls), dtype=torch.int64, device=clu.device) if want_hist else None
  ws = workspace(lib().spml_segment_majority_workspace_bytes(m, ncls), clu.device)
  check(lib().spml_segment_majority_i64(ptr(clu, torch.int64), ptr(sem, torch.int64), p, m, ncls,
                                        ptr(major), ptr(hist, None, True), ptr(ws), ws.numel(), stream_ptr()),
        'spml_segment_majority_i64')
  return (major, hist) if want_hist else major


# ---------------------------------------------------------------------------
# tag-recipe kNN pseudo labels: tag-normalised arg-max (csrc/tag_normalize.hip)
MAX_TAG_NORMALIZE_CLASSES = 64         # the limit of spml_tag_normalize_argmax_f32 (include/spml_hip.h)


def tag_normalize_argmax(acc, num_views, tags, floor=0.15, want_prob=False):
  """The tail of pseudo_inference_crf_msc.py:252-263,275 on `acc` fp32 `[ncls, h, w]`, the SUM of the vote maps of
  `num_views` views (what `view_votes_accumulate` leaves; only read): mean over the views, per class the maximum over the
  image, floored at `floor`, 1 where `tags` (bool or uint8 `[ncls]`) is false, the division, the arg-max (ties to the
  lowest class).  -> (labels int64 `[h, w]`, prob fp32 `[ncls, h, w]` or None, divisor fp32 `[ncls]`).  All tensors
  contiguous, on the GPU; two launches, no host read."""
  if acc.dim() != 3 or tags.dim() != 1 or tags.shape[0] != acc.shape[0]:
    raise SpmlHipError('tag_normalize_argmax: acc must be [ncls, h, w] and tags [ncls] (got %s, %s)'
                       % (tuple(acc.shape), tuple(tags.shape)))
  if tags.dtype not in (torch.bool, torch.uint8):
    raise SpmlHipError('tag_normalize_argmax: tags must be bool or uint8 (got %s)' % tags.dtype)
  ncls, h, w = (int(v) for v in acc.shape)
  ptr(acc, torch.float32), ptr(tags)                         # (CPU tensors are refused before anything is allocated)
  nbytes = lib().spml_tag_normalize_workspace_bytes(ncls, h * w)
  if nbytes == 0:
    raise SpmlHipError('tag_normalize_argmax: %d classes x %d pixels are outside the kernel (1 .. %d classes, at least '
                       'one pixel)' % (ncls, h * w, MAX_TAG_NORMALIZE_CLASSES))
  tags8 = tags.view(torch.uint8) if tags.dtype == torch.bool else tags
  labels = torch.empty((h, w), dtype=torch.int64, device=acc.device)
  prob = torch.empty_like(acc) if want_prob else None
  divisor = torch.empty((ncls,), dtype=torch.float32, device=acc.device)
  ws = workspace(nbytes, acc.device)
  check(lib().spml_tag_normalize_argmax_f32(ptr(acc, torch.float32), ncls, h * w, int(num_views), ptr(tags8, torch.uint8),
                                            float(floor), ptr(labels), ptr(prob, None, True), ptr(divisor), ptr(ws),
                                            ws.numel(), stream_ptr()), 'spml_tag_normalize_argmax_f32')
  return labels, prob, divisor


def affinity_transition(emb, scale=5.0, power=20):
  """emb [B,C,n] (unit columns) -> column-stochastic transition matrix [n,n]."""
  b, c, n = emb.shape
  trans = torch.empty((n, n), dtype=torch.float32, device=emb.device)
  ws = workspace(lib().spml_affinity_workspace_bytes(b, c, n), emb.device)
  check(lib().spml_affinity_transition_f32(
      ptr(emb, torch.float32), b, c, n, float(scale), int(power), ptr(trans), ptr(ws), ws.numel(),
      stream_ptr()), 'spml_affinity_transition_f32')
  return trans


# ---------------------------------------------------------------------------
# fused batch norm + ReLU + residual (channels-last [R, C] views of NHWC tensors)
def _nhwc_rows(t):
  """(R, C) of a 4-D channels-last tensor (or a 2-D [R, C] one)."""
  if t.dim() == 2:
    return t.shape[0], t.shape[1]
  n, c, h, w = t.shape
  if not t.is_contiguous(memory_format=torch.channels_last):
    raise SpmlHipError('fused batch norm needs channels-last (NHWC) tensors')
  return n * h * w, c


def _ptr_any(t, allow_none=False):
  """data_ptr of a CUDA fp32 tensor that is dense in memory (NCHW-contiguous or channels-last)."""
  if t is None:
    if allow_none:
      return c_void_p(0)
    raise SpmlHipError('missing tensor argument')
  if not t.is_cuda or t.dtype != torch.float32:
    raise SpmlHipError('expected a float32 GPU tensor (got %s on %s)' % (t.dtype, t.device))
  if t.device.index != torch.cuda.current_device():
    raise SpmlHipError('tensor lives on %s but the current device is cuda:%d' % (t.device, torch.cuda.current_device()))
  return c_void_p(t.data_ptr())


def _stream_workspace(cache, need, device):
  """Scratch of at least `need` bytes, cached per (device, current stream): reuse is stream-ordered (every call
  consumes its scratch before the next one on the same stream overwrites it), and two streams never share a buffer."""
  key = (device.index, torch.cuda.current_stream().cuda_stream)
  ws = cache.get(key)
  if ws is None or ws.numel() < need:
    ws = cache[key] = workspace(need, device)
  return ws


_bn_ws = {}


def _bn_workspace(r, c, device):
  """Cached scratch for the batch-norm partial sums."""
  return _stream_workspace(_bn_ws, lib().spml_bn_workspace_bytes(r, c), device)


def bn_act_fwd(x, residual, gamma, beta, running_mean, running_var, momentum, eps, relu):
  """Single-rank fused forward -> (y, mean, invstd); updates the running statistics in place."""
  r, c = _nhwc_rows(x)
  y = torch.empty_like(x)
  stats = torch.empty((2, c), dtype=torch.float32, device=x.device)
  ws = _bn_workspace(r, c, x.device)
  check(lib().spml_bn_act_fwd_f32(
      _ptr_any(x), _ptr_any(residual, True), r, c, ptr(gamma, torch.float32), ptr(beta, torch.float32),
      ptr(running_mean, None, True), ptr(running_var, None, True), float(momentum), float(eps),
      int(bool(relu)), _ptr_any(y), c_void_p(stats[0].data_ptr()), c_void_p(stats[1].data_ptr()), ptr(ws),
      ws.numel(), stream_ptr()), 'spml_bn_act_fwd_f32')
  return y, stats[0], stats[1]


def bn_act_bwd(dy, y, x, mean, invstd, gamma, want_dx=True, want_dres=False):
  """Single-rank fused backward -> (dx, d_residual, d_gamma, d_beta)."""
  r, c = _nhwc_rows(dy)
  dx = torch.empty_like(dy) if want_dx else None
  dres = torch.empty_like(dy) if want_dres else None
  dgb = torch.empty((2, c), dtype=torch.float32, device=dy.device)
  ws = _bn_workspace(r, c, dy.device)
  check(lib().spml_bn_act_bwd_f32(
      _ptr_any(dy), _ptr_any(y, True), _ptr_any(x), r, c, c_void_p(mean.data_ptr()), c_void_p(invstd.data_ptr()),
      ptr(gamma, torch.float32), c_void_p(dgb[0].data_ptr()), c_void_p(dgb[1].data_ptr()), _ptr_any(dx, True),
      _ptr_any(dres, True), ptr(ws), ws.numel(), stream_ptr()), 'spml_bn_act_bwd_f32')
  return dx, dres, dgb[0], dgb[1]


def bn_stats(x):
  r, c = _nhwc_rows(x)
  mean = torch.empty((c,), dtype=torch.float32, device=x.device)
  m2 = torch.empty((c,), dtype=torch.float32, device=x.device)
  ws = workspace(lib().spml_bn_workspace_bytes(r, c), x.device)
  check(lib().spml_bn_stats_f32(_ptr_any(x), r, c, ptr(mean), ptr(m2), ptr(ws), ws.numel(), stream_ptr()),
        'spml_bn_stats_f32')
  return mean, m2


def bn_act_apply(x, residual, mean, invstd, gamma, beta, relu):
  r, c = _nhwc_rows(x)
  y = torch.empty_like(x)
  check(lib().spml_bn_act_apply_f32(_ptr_any(x), _ptr_any(residual, True), r, c, ptr(mean), ptr(invstd),
                                    ptr(gamma, torch.float32), ptr(beta, torch.float32), int(bool(relu)),
                                    _ptr_any(y), stream_ptr()), 'spml_bn_act_apply_f32')
  return y


def bn_act_bwd_reduce(dy, y, x, mean, invstd):
  r, c = _nhwc_rows(x)
  s0 = torch.empty((c,), dtype=torch.float32, device=x.device)
  s1 = torch.empty((c,), dtype=torch.float32, device=x.device)
  ws = workspace(lib().spml_bn_workspace_bytes(r, c), x.device)
  check(lib().spml_bn_act_bwd_reduce_f32(_ptr_any(dy), _ptr_any(y, True), _ptr_any(x), r, c, ptr(mean),
                                         ptr(invstd), ptr(s0), ptr(s1), ptr(ws), ws.numel(), stream_ptr()),
        'spml_bn_act_bwd_reduce_f32')
  return s0, s1


def bn_act_bwd_apply(dy, y, x, mean, invstd, gamma, sum_dz, sum_dz_xhat, count, want_dx=True,
                     want_dres=False):
  """count: rows the statistics were pooled over -- a number, or the device float [1] that
  bn_finalize_ranks wrote (SyncBatchNorm: the ranks' row counts may differ)."""
  r, c = _nhwc_rows(dy)
  count, count_dev = _count_args(count)
  dx = torch.empty_like(dy) if want_dx else None
  dres = torch.empty_like(dy) if want_dres else None
  check(lib().spml_bn_act_bwd_apply_f32(
      _ptr_any(dy), _ptr_any(y, True), _ptr_any(x, True), r, c, ptr(mean, None, True), ptr(invstd, None, True),
      ptr(gamma, None, True), ptr(sum_dz, None, True), ptr(sum_dz_xhat, None, True), count, count_dev,
      _ptr_any(dx, True), _ptr_any(dres, True), stream_ptr()), 'spml_bn_act_bwd_apply_f32')
  return dx, dres


# ---------------------------------------------------------------------------
# split-f16 ("hl8") tensors and the matrix-core convolutions (csrc/conv.hip)
# ---------------------------------------------------------------------------

class Hl8(object):
  """Split-f16 copy of an fp32 tensor [rows, C]: `data` (uint8, rows*C*4 bytes) + the device
  float `bound` (>= max|v|, fixes the power-of-two scale) -- see include/spml_hip.h."""
  __slots__ = ('data', 'bound', 'rows', 'channels')

  def __init__(self, data, bound, rows, channels):
    self.data, self.bound, self.rows, self.channels = data, bound, rows, channels


def hl8_from_f32(x, rows=None, channels=None, bound=None):
  """x: dense fp32 GPU tensor read as [rows, channels] (default: channels-last 4-D or 2-D)."""
  if rows is None:
    rows, channels = _nhwc_rows(x)
  compute = bound is None
  if compute:
    bound = torch.empty((1,), dtype=torch.float32, device=x.device)
  out = torch.empty((rows * channels * 4,), dtype=torch.uint8, device=x.device)
  check(lib().spml_hl8_from_f32(_ptr_any(x), rows, channels, c_void_p(bound.data_ptr()), int(compute),
                                ptr(out), stream_ptr()), 'spml_hl8_from_f32')
  return Hl8(out, bound, rows, channels)


def hl8_weight(w):
  """Conv weight [Cout, Cin, kh, kw] -> (forward operand [Cout][taps*Cin], data-gradient operand
  [Cin][taps*Cout] with mirrored taps); both share one scale."""
  cout, cin, kh, kw = w.shape
  taps = kh * kw
  wl = w.detach().contiguous(memory_format=torch.channels_last)          # [Cout][kh][kw][Cin] storage
  fwd = hl8_from_f32(wl, cout, taps * cin)
  tr = torch.empty((cout * taps * cin * 4,), dtype=torch.uint8, device=w.device)
  check(lib().spml_hl8_weight_transposed_f32(_ptr_any(wl), cout, taps, cin, c_void_p(fwd.bound.data_ptr()),
                                             ptr(tr), stream_ptr()), 'spml_hl8_weight_transposed_f32')
  return fwd, Hl8(tr, fwd.bound, cin, taps * cout)


@functools.lru_cache(maxsize=None)         # (a pure function of the three numbers, asked per unit and forward)
def conv_hl8_supported(k, n, taps):
  return bool(lib().spml_conv_hl8_supported(int(k), int(n), int(taps)))


def _conv_operands(who, a, b, n_img, h, w, taps):
  """Head of the conv_hl8* wrappers (`who`): a Hl8 [n_img*h*w, K], b Hl8 [N, taps*K] -> (K, N, the output
  [n_img, N, h, w] channels-last fp32, the four operand pointers a, a_bound, b, b_bound)."""
  k, n = a.channels, b.rows
  if a.rows != n_img * h * w or b.channels != taps * k:
    raise SpmlHipError('%s: operand shapes do not match' % who)
  out = torch.empty((n_img, n, h, w), dtype=torch.float32, device=a.data.device, memory_format=torch.channels_last)
  return k, n, out, (ptr(a.data), c_void_p(a.bound.data_ptr()), ptr(b.data), c_void_p(b.bound.data_ptr()))


def conv_hl8(a, b, n_img, h, w, taps, dilation=1, addend=None, addend_mask=None):
  """out [n_img, N, h, w] (channels-last fp32) = conv(a, b): a Hl8 [n_img*h*w, K], b Hl8 [N, taps*K]."""
  k, n, out, operands = _conv_operands('conv_hl8', a, b, n_img, h, w, taps)
  check(lib().spml_conv_hl8_f32(*operands, _ptr_any(addend, True), _dp(addend_mask), _ptr_any(out), n_img, h, w,
                                k, n, taps, dilation, stream_ptr()), 'spml_conv_hl8_f32')
  return out


class ChunkStats(object):
  """Per-row-tile column statistics a convolution's epilogue left for the batch norm that follows:
  data [4, chunks, N] (mean, M2, max, min), chunk geometry, and the bound slot the launch reset."""

  def __init__(self, data, chunks, chunk_rows, bound):
    self.data, self.chunks, self.chunk_rows, self.bound = data, chunks, chunk_rows, bound


def conv_hl8_stats(a, b, n_img, h, w, taps, dilation=1):
  """conv_hl8 whose epilogue also leaves the chunk statistics of the output -> (out, ChunkStats), or
  (out, None) where the launch has no per-tile column owner (narrow outputs).  SPML_CONV_BN_STATS=0: never."""
  chunks, rows = ctypes.c_int(0), ctypes.c_int(0)
  if os.environ.get('SPML_CONV_BN_STATS') == '0' or lib().spml_conv_hl8_stats_layout(
      n_img, h, w, a.channels, b.rows, taps, ctypes.byref(chunks), ctypes.byref(rows)) != 0:
    return conv_hl8(a, b, n_img, h, w, taps, dilation), None
  k, n, out, operands = _conv_operands('conv_hl8_stats', a, b, n_img, h, w, taps)
  st = torch.empty((4, chunks.value, n), dtype=torch.float32, device=out.device)
  bound = _f32(1, out.device)
  check(lib().spml_conv_hl8_stats_f32(*operands, _ptr_any(out), _dp(st), _dp(bound), n_img, h, w, k, n, taps,
                                      dilation, stream_ptr()), 'spml_conv_hl8_stats_f32')
  return out, ChunkStats(st, chunks.value, rows.value, bound)


def conv_hl8_bwd_stats(a, b, n_img, h, w, taps, dilation, bn_x, relu_mask, bn_mean, addend=None, addend_mask=None):
  """conv_hl8 as the data gradient in front of a batch norm + ReLU (saved input bn_x, mask bytes, batch mean): the
  epilogue also leaves that batch norm's backward chunk sums -> (out, ChunkStats [3, chunks, N]), or (out, None)
  where the launch has no per-tile column owner (narrow outputs) or there is no mask.  SPML_CONV_BN_BWD_STATS=0:
  never.  addend (+ addend_mask): added to the result as conv_hl8 does, before the sums are taken (a unit's last data
  gradient in front of the bn3 of the unit below); launches with the chunked accumulation take the plain route."""
  k, n = a.channels, b.rows
  chunks, rows = ctypes.c_int(0), ctypes.c_int(0)
  if relu_mask is None or os.environ.get('SPML_CONV_BN_BWD_STATS') == '0' or lib().spml_conv_hl8_bwd_stats_layout(
      n_img, h, w, k, n, taps, ctypes.byref(chunks), ctypes.byref(rows)) != 0 or \
      (addend is not None and 'chunk' in conv_hl8_path_name('bwd_stats', n_img, h, w, k, n, taps)):
    return conv_hl8(a, b, n_img, h, w, taps, dilation, addend, addend_mask), None
  if bn_x.numel() != a.rows * n or relu_mask.numel() != a.rows * (n // 4) or bn_mean.numel() != n or \
      (addend is not None and addend.numel() != a.rows * n) or (addend is None and addend_mask is not None) or \
      (addend_mask is not None and addend_mask.numel() != a.rows * (n // 4)):
    raise SpmlHipError('conv_hl8_bwd_stats: operand shapes do not match')
  k, n, out, operands = _conv_operands('conv_hl8_bwd_stats', a, b, n_img, h, w, taps)
  st = torch.empty((3, chunks.value, n), dtype=torch.float32, device=out.device)
  bound = _f32(1, out.device)
  args = operands + (_ptr_any(out), _ptr_any(bn_x), _dp(relu_mask), _dp(bn_mean), _dp(st), _dp(bound), n_img, h, w,
                     k, n, taps, dilation)
  if addend is None:
    check(lib().spml_conv_hl8_bwd_stats_f32(*args, stream_ptr()), 'spml_conv_hl8_bwd_stats_f32')
  else:
    check(lib().spml_conv_hl8_bwd_stats_addend_f32(*args, _ptr_any(addend), _dp(addend_mask), stream_ptr()),
          'spml_conv_hl8_bwd_stats_addend_f32')
  return out, ChunkStats(st, chunks.value, rows.value, bound)


CONV_ENTRIES = {'plain': 0, 'stats': 1, 'bwd_stats': 2, 'affine': 3, 'pyramid': 4}


def conv_hl8_path_name(entry, n_img, h, w, k, n, taps_or_groups, has_addend=False):
  """conv_gemm instantiation the entry point ('plain', 'stats', 'bwd_stats', 'affine', 'pyramid': there
  taps_or_groups = groups) launches for a shape under the current environment and deterministic mode -- a pure
  host function of the library, the launch's own expression; names: include/spml_hip.h."""
  return lib().spml_conv_hl8_path_name(CONV_ENTRIES[entry], int(n_img), int(h), int(w), int(k), int(n),
                                       int(taps_or_groups), int(bool(has_addend))).decode()


def conv_wgrad_path_name(n_img, h, w, k, n, taps_or_branches, pyramid=False):
  """conv_wgrad instantiation of the weight gradient (pyramid: taps_or_branches = branches)."""
  return lib().spml_conv_wgrad_path_name(int(n_img), int(h), int(w), int(k), int(n), int(taps_or_branches),
                                         int(bool(pyramid))).decode()


def conv_wgrad_splits(n_img, h, w, k, n, taps_or_branches, pyramid=False):
  """Workgroups per tile over the pixel range of that launch (0: unsupported)."""
  return lib().spml_conv_wgrad_splits(int(n_img), int(h), int(w), int(k), int(n), int(taps_or_branches),
                                      int(bool(pyramid)))


@functools.lru_cache(maxsize=None)
def conv_wgrad_hl8_supported(k, n, taps):
  return bool(lib().spml_conv_wgrad_hl8_supported(int(k), int(n), int(taps)))


_wgrad_ws = {}


def conv_wgrad_hl8(dy, x, n_img, h, w, taps, dilation=1):
  """dW [N, K, kh, kw] (channels-last storage [N][taps][K]) from dy Hl8 [R, N] and x Hl8 [R, K]."""
  n, k = dy.channels, x.channels
  if dy.rows != n_img * h * w or x.rows != dy.rows:
    raise SpmlHipError('conv_wgrad_hl8: operand shapes do not match')
  ws = _stream_workspace(_wgrad_ws, lib().spml_conv_wgrad_workspace_bytes(n_img, h, w, k, n, taps), dy.data.device)
  side = 3 if taps == 9 else 1
  dw = torch.empty((n, k, side, side), dtype=torch.float32, device=dy.data.device,
                   memory_format=torch.channels_last)
  check(lib().spml_conv_wgrad_hl8_f32(ptr(dy.data), c_void_p(dy.bound.data_ptr()), ptr(x.data),
                                      c_void_p(x.bound.data_ptr()), _ptr_any(dw), n_img, h, w, k, n, taps,
                                      dilation, ptr(ws), ws.numel(), stream_ptr()), 'spml_conv_wgrad_hl8_f32')
  return dw


def conv_wgrad_pyramid_hl8_supported(k, n, branches):
  return bool(lib().spml_conv_wgrad_pyramid_hl8_supported(int(k), int(n), int(branches)))


def conv_wgrad_pyramid_hl8(dy, x, n_img, h, w, dilations):
  """The weight gradients of up to four dilated 3x3 branches (64 output channels each) that share the output
  gradient dy Hl8 [R, 64], from x Hl8 [R, K]: a list of dW [64, K, 3, 3] (channels-last storage), views of one
  [branches, 64, 9, K] buffer written by one launch."""
  n, k, nb = dy.channels, x.channels, len(dilations)
  if dy.rows != n_img * h * w or x.rows != dy.rows:
    raise SpmlHipError('conv_wgrad_pyramid_hl8: operand shapes do not match')
  need = lib().spml_conv_wgrad_pyramid_workspace_bytes(n_img, h, w, k, n, nb)
  if need == 0:
    raise SpmlHipError('conv_wgrad_pyramid_hl8: unsupported shape (K %d, N %d, %d branches)' % (k, n, nb))
  ws = _stream_workspace(_wgrad_ws, need, dy.data.device)
  dw = torch.empty((nb, n, 3, 3, k), dtype=torch.float32, device=dy.data.device)
  dil = (ctypes.c_int * nb)(*[int(d) for d in dilations])
  check(lib().spml_conv_wgrad_pyramid_hl8_f32(ptr(dy.data), c_void_p(dy.bound.data_ptr()), ptr(x.data),
                                              c_void_p(x.bound.data_ptr()), _ptr_any(dw), n_img, h, w, k, n, nb,
                                              ctypes.cast(dil, c_void_p), ptr(ws), ws.numel(), stream_ptr()),
        'spml_conv_wgrad_pyramid_hl8_f32')
  return [dw[b].permute(0, 3, 1, 2) for b in range(nb)]


def _f32(n, device):
  return torch.empty((n,), dtype=torch.float32, device=device)


def _dp(t):
  return c_void_p(0) if t is None else c_void_p(t.data_ptr())


def bn_stats_ext(x, rows, channels, chunk_stats=None):
  """Local statistics of x read as [rows, channels] fp32 -> [5, C] = (count, mean, M2, channel max,
  channel min); rows 0..2 are what the ranks exchange.  chunk_stats: pooled from the statistics the
  producing convolution's epilogue left instead of reading x."""
  st = torch.empty((5, channels), dtype=torch.float32, device=x.device)
  st[0].fill_(float(rows))
  if chunk_stats is not None:
    check(lib().spml_bn_stats_ext_chunks_f32(_dp(chunk_stats.data), chunk_stats.chunks, chunk_stats.chunk_rows, rows,
                                             channels, _dp(st[1]), _dp(st[2]), _dp(st[3]), _dp(st[4]), stream_ptr()),
          'spml_bn_stats_ext_chunks_f32')
    return st
  ws = _bn_workspace(rows, channels, x.device)
  check(lib().spml_bn_stats_ext_f32(_ptr_any(x), rows, channels, _dp(st[1]), _dp(st[2]), _dp(st[3]), _dp(st[4]),
                                    ptr(ws), ws.numel(), stream_ptr()), 'spml_bn_stats_ext_f32')
  return st


def _count_args(count):
  """(host count, device count pointer) of the batch-norm backward apply calls."""
  if torch.is_tensor(count):
    return 0.0, ptr(count, torch.float32)
  return float(count), None


def bn_finalize_ranks(gathered, eps, momentum, running_mean, running_var):
  """gathered [world, 3, C] (count, mean, M2 per rank) -> pooled (mean, invstd, total row count [1], a
  device float: the ranks' counts are never read on the host); running statistics updated."""
  world, _, c = gathered.shape
  out = torch.empty((2 * c + 4,), dtype=torch.float32, device=gathered.device)
  mean, invstd, total = out[:c], out[c:2 * c], out[2 * c:2 * c + 1]
  check(lib().spml_bn_finalize_ranks_f32(ptr(gathered, torch.float32), world, c, float(eps), float(momentum),
                                         _dp(running_mean), _dp(running_var), _dp(mean), _dp(invstd), _dp(total),
                                         stream_ptr()),
        'spml_bn_finalize_ranks_f32')
  return mean, invstd, total


def bn_finalize(mean, m2, count, eps, momentum, running_mean, running_var):
  invstd = torch.empty_like(mean)
  check(lib().spml_bn_finalize_f32(_dp(mean), _dp(m2), mean.numel(), float(count), float(eps), float(momentum),
                                   _dp(running_mean), _dp(running_var), _dp(invstd), stream_ptr()),
        'spml_bn_finalize_f32')
  return invstd


def bn_act_apply_hl8(x, rows, channels, residual, residual_bound, mean, invstd, gamma, beta, cmax, cmin, relu,
                     want_f32, want_hl8, like=None, want_mask=False):
  """-> (y fp32 or None, Hl8 or None, bound, ReLU mask bytes or None)"""
  y = torch.empty_like(x if like is None else like) if want_f32 else None
  yh = torch.empty((rows * channels * 4,), dtype=torch.uint8, device=x.device) if want_hl8 else None
  bound = _f32(1, x.device)
  mask = torch.empty((rows * (channels // 4),), dtype=torch.uint8, device=x.device) if want_mask else None
  check(lib().spml_bn_act_apply_hl8_f32(
      _ptr_any(x), _ptr_any(residual, True), _dp(residual_bound), rows, channels, _dp(mean), _dp(invstd),
      ptr(gamma, torch.float32), ptr(beta, torch.float32), _dp(cmax), _dp(cmin), int(bool(relu)), _ptr_any(y, True),
      _dp(yh), _dp(bound), _dp(mask), stream_ptr()), 'spml_bn_act_apply_hl8_f32')
  return y, (Hl8(yh, bound, rows, channels) if want_hl8 else None), bound, mask


def bn_act_bwd_reduce_ext(dy, y, relu_mask, x, rows, channels, mean, invstd, chunk_stats=None):
  """-> (sum dz, sum dz*xhat, max|dz| per channel); ReLU mask from y (fp32), the mask bytes or none.
  chunk_stats: pooled from the chunk sums the producing data gradient's epilogue left (`conv_hl8_bwd_stats`)
  instead of reading dy and x."""
  st = torch.empty((3, channels), dtype=torch.float32, device=dy.device)     # rows 0, 1 are all-reduced together
  if chunk_stats is not None:
    check(lib().spml_bn_act_bwd_reduce_ext_chunks_f32(
        _dp(chunk_stats.data), chunk_stats.chunks, chunk_stats.chunk_rows, rows, channels, _dp(invstd), _dp(st[0]),
        _dp(st[1]), _dp(st[2]), stream_ptr()), 'spml_bn_act_bwd_reduce_ext_chunks_f32')
    return st
  ws = _bn_workspace(rows, channels, dy.device)
  check(lib().spml_bn_act_bwd_reduce_ext_f32(
      _ptr_any(dy), _ptr_any(y, True), _dp(relu_mask), _ptr_any(x), rows, channels,
      _dp(mean), _dp(invstd), _dp(st[0]), _dp(st[1]), _dp(st[2]), ptr(ws), ws.numel(), stream_ptr()),
        'spml_bn_act_bwd_reduce_ext_f32')
  return st


def bn_act_bwd_apply_hl8(dy, y, relu_mask, x, rows, channels, mean, invstd, gamma, s0, s1, max_dz, cmax, cmin, count,
                         want_dx_f32=False, want_dx_hl8=True, want_dres=False):
  """-> (dx fp32 or None, dx Hl8 or None, d_residual fp32 or None)"""
  dx = torch.empty_like(dy) if want_dx_f32 else None
  dxh = torch.empty((rows * channels * 4,), dtype=torch.uint8, device=dy.device) if want_dx_hl8 else None
  bound = _f32(1, dy.device) if want_dx_hl8 else None
  dres = torch.empty_like(dy) if want_dres else None
  count, count_dev = _count_args(count)
  check(lib().spml_bn_act_bwd_apply_hl8_f32(
      _ptr_any(dy), _ptr_any(y, True), _dp(relu_mask), _ptr_any(x), rows, channels,
      _dp(mean), _dp(invstd), ptr(gamma, torch.float32), _dp(s0), _dp(s1), _dp(max_dz), _dp(cmax), _dp(cmin),
      count, count_dev, _ptr_any(dx, True), _dp(dxh), _dp(bound), _ptr_any(dres, True), stream_ptr()),
        'spml_bn_act_bwd_apply_hl8_f32')
  return dx, (Hl8(dxh, bound, rows, channels) if want_dx_hl8 else None), dres


def bn_fwd_hl8(x, rows, channels, residual, residual_bound, gamma, beta, running_mean, running_var, momentum, eps,
               relu, want_f32, want_hl8, want_mask, chunk_stats=None):
  """Single-rank batch norm forward -> (y fp32|None, Hl8|None, bound, mask|None, saved (mean, invstd, cmax, cmin))."""
  y = torch.empty_like(x) if want_f32 else None
  yh = torch.empty((rows * channels * 4,), dtype=torch.uint8, device=x.device) if want_hl8 else None
  bound = _f32(1, x.device) if chunk_stats is None else chunk_stats.bound
  mask = torch.empty((rows * (channels // 4),), dtype=torch.uint8, device=x.device) if want_mask else None
  st = torch.empty((4, channels), dtype=torch.float32, device=x.device)
  if chunk_stats is not None:              # the producing convolution already took the statistics
    check(lib().spml_bn_fwd_hl8_chunks_f32(
        _ptr_any(x), _dp(chunk_stats.data), chunk_stats.chunks, chunk_stats.chunk_rows, _ptr_any(residual, True),
        _dp(residual_bound), rows, channels, ptr(gamma, torch.float32), ptr(beta, torch.float32), _dp(running_mean),
        _dp(running_var), float(momentum), float(eps), int(bool(relu)), _ptr_any(y, True), _dp(yh), _dp(bound),
        _dp(mask), _dp(st[0]), _dp(st[1]), _dp(st[2]), _dp(st[3]), stream_ptr()), 'spml_bn_fwd_hl8_chunks_f32')
  else:
    ws = _bn_workspace(rows, channels, x.device)
    check(lib().spml_bn_fwd_hl8_f32(
        _ptr_any(x), _ptr_any(residual, True), _dp(residual_bound), rows, channels, ptr(gamma, torch.float32),
        ptr(beta, torch.float32), _dp(running_mean), _dp(running_var), float(momentum), float(eps), int(bool(relu)),
        _ptr_any(y, True), _dp(yh), _dp(bound), _dp(mask), _dp(st[0]), _dp(st[1]), _dp(st[2]), _dp(st[3]), ptr(ws),
        ws.numel(), stream_ptr()), 'spml_bn_fwd_hl8_f32')
  return y, (Hl8(yh, bound, rows, channels) if want_hl8 else None), bound, mask, (st[0], st[1], st[2], st[3])


def bn_bwd_hl8(dy, relu_mask, x, rows, channels, saved, gamma, want_dres=False, chunk_stats=None):
  """Single-rank batch norm backward -> (dx Hl8, d_residual|None, d_gamma, d_beta).  chunk_stats: the chunk sums the
  producer of dy left (`conv_hl8_bwd_stats`, which also reset their bound slot): dy and x are read once."""
  mean, invstd, cmax, cmin = saved
  dxh = torch.empty((rows * channels * 4,), dtype=torch.uint8, device=dy.device)
  dres = torch.empty_like(dy) if want_dres else None
  if chunk_stats is not None:
    bound = chunk_stats.bound
    dgb = torch.empty((3, channels), dtype=torch.float32, device=dy.device)      # d_gamma, d_beta, max |dz|
    check(lib().spml_bn_bwd_hl8_chunks_f32(
        _ptr_any(dy), _dp(relu_mask), _ptr_any(x), _dp(chunk_stats.data), chunk_stats.chunks, chunk_stats.chunk_rows,
        rows, channels, _dp(mean), _dp(invstd), ptr(gamma, torch.float32), _dp(cmax), _dp(cmin), _dp(dgb[0]),
        _dp(dgb[1]), _dp(dgb[2]), c_void_p(0), _dp(dxh), _dp(bound), _ptr_any(dres, True), stream_ptr()),
          'spml_bn_bwd_hl8_chunks_f32')
  else:
    bound = _f32(1, dy.device)
    dgb = torch.empty((2, channels), dtype=torch.float32, device=dy.device)
    ws = _bn_workspace(rows, channels, dy.device)
    check(lib().spml_bn_bwd_hl8_f32(
        _ptr_any(dy), c_void_p(0), _dp(relu_mask), _ptr_any(x), rows, channels, _dp(mean), _dp(invstd),
        ptr(gamma, torch.float32), _dp(cmax), _dp(cmin), _dp(dgb[0]), _dp(dgb[1]), c_void_p(0), _dp(dxh), _dp(bound),
        _ptr_any(dres, True), ptr(ws), ws.numel(), stream_ptr()), 'spml_bn_bwd_hl8_f32')
  return Hl8(dxh, bound, rows, channels), dres, dgb[0], dgb[1]


def conv_hl8_pyramid_dgrad(dy, weights, dilations, n_img, h, w):
  """dX of `sum_g conv2d(x, weights[g], dilation=dilations[g], padding=dilations[g])` for 3x3 weights
  [Cout, Cin, 3, 3] sharing the output gradient dy (Hl8 [R, Cout]) -> fp32 [n_img, Cin, h, w]."""
  groups = len(weights)
  cout, cin = weights[0].shape[0], weights[0].shape[1]
  dev = dy.data.device
  bound = torch.empty((1,), dtype=torch.float32, device=dev)
  wl = [wt.detach().contiguous(memory_format=torch.channels_last) for wt in weights]
  for g, wt in enumerate(wl):
    check(lib().spml_absmax_bound_f32(_ptr_any(wt), wt.numel(), _dp(bound), int(g == 0), stream_ptr()),
          'spml_absmax_bound_f32')
  b = torch.empty((cin * 9 * groups * cout * 4,), dtype=torch.uint8, device=dev)
  for g, wt in enumerate(wl):
    check(lib().spml_hl8_weight_transposed_into_f32(_ptr_any(wt), cout, 9, cin, _dp(bound), ptr(b), 9 * groups, 9 * g,
                                                    stream_ptr()), 'spml_hl8_weight_transposed_into_f32')
  out = torch.empty((n_img, cin, h, w), dtype=torch.float32, device=dev, memory_format=torch.channels_last)
  dil = (ctypes.c_int * 4)(*([int(d) for d in dilations] + [1] * (4 - groups)))
  check(lib().spml_conv_hl8_pyramid_f32(ptr(dy.data), _dp(dy.bound), ptr(b), _dp(bound), c_void_p(0), c_void_p(0),
                                        _ptr_any(out), n_img, h, w, cout, cin, groups, dil, stream_ptr()),
        'spml_conv_hl8_pyramid_f32')
  return out


def conv_hl8_pyramid_forward(x, weights, biases, dilations, n_img, h, w):
  """sum_g conv2d(x, weights[g], biases[g], dilation = padding = dilations[g]) for 3x3 weights
  [Cout, Cin, 3, 3] in one launch (x: Hl8 [R, Cin]) -> fp32 [n_img, Cout, h, w]."""
  groups = len(weights)
  cout, cin = weights[0].shape[0], weights[0].shape[1]
  dev = x.data.device
  # forward operand [Cout][36 taps * Cin]: the branches' channels-last weights side by side
  cat = torch.cat([wt.detach().permute(0, 2, 3, 1).reshape(cout, 9 * cin) for wt in weights], dim=1).contiguous()
  b = hl8_from_f32(cat, cout, 9 * groups * cin)
  bias = None
  if any(bb is not None for bb in biases):
    bias = sum(bb.detach() for bb in biases if bb is not None).contiguous()
  out = torch.empty((n_img, cout, h, w), dtype=torch.float32, device=dev, memory_format=torch.channels_last)
  dil = (ctypes.c_int * 4)(*([int(d) for d in dilations] + [1] * (4 - groups)))
  check(lib().spml_conv_hl8_pyramid_f32(ptr(x.data), _dp(x.bound), ptr(b.data), _dp(b.bound), _dp(bias), c_void_p(0),
                                        _ptr_any(out), n_img, h, w, cin, cout, groups, dil, stream_ptr()),
        'spml_conv_hl8_pyramid_f32')
  return out


_pyramid_operand_cache = {}     # the last packed operand of conv_hl8_pyramid_forward_gemm (one head per model)


def conv_hl8_pyramid_forward_gemm_supported(cin, cout, groups):
  return (16 <= cout <= 1024 and cout & (cout - 1) == 0 and 1 <= groups <= 4 and
          conv_hl8_supported(cin, 9 * groups * cout, 1))


def conv_hl8_pyramid_forward_gemm(x, weights, biases, dilations, n_img, h, w):
  """The same sum of dilated 3x3 branches as `conv_hl8_pyramid_forward`, for narrow heads: ONE 1x1 convolution
  with 9 * branches * Cout columns (z[r][tap * Cout + n] = x[r] . w_tap[n]: x is streamed once per 256 columns
  instead of once per tap) + `spml_conv_tap_gather_f32`, which adds every output pixel's taps from their shifted
  rows of z in a fixed order."""
  groups = len(weights)
  cout, cin = weights[0].shape[0], weights[0].shape[1]
  dev = x.data.device
  # 1x1 operand [(branch, kh, kw, n)][Cin]: packed once per version of the weights (inference re-uses it; a training
  # step changes the weights in place -- `_version` moves -- and packs again)
  # (the key holds WEAK references to the weight tensors themselves: a pointer + version pair alone can recur for a
  # different tensor once the first one has been freed -- it did, in the test suite)
  import weakref
  refs, vers = _pyramid_operand_cache.get('refs', ()), _pyramid_operand_cache.get('versions', ())
  if (len(refs) == groups and all(r() is wt for r, wt in zip(refs, weights)) and
      vers == tuple(wt._version for wt in weights)):
    operand = _pyramid_operand_cache['operand']
  else:
    cat = torch.stack([wt.detach().permute(2, 3, 0, 1).reshape(9 * cout, cin) for wt in weights]).reshape(
        9 * groups * cout, cin).contiguous()
    operand = hl8_from_f32(cat, 9 * groups * cout, cin)
    _pyramid_operand_cache.update(refs=tuple(weakref.ref(wt) for wt in weights),
                                  versions=tuple(wt._version for wt in weights), operand=operand)
  # (z is [rows, 9 * branches * Cout] fp32 -- 623 MB at batch 16, 65 x 65, 2304 columns -- alive until the gather below)
  z = conv_hl8(x, operand, n_img, h, w, 1)
  bias = None
  if any(bb is not None for bb in biases):
    bias = sum(bb.detach() for bb in biases if bb is not None).contiguous()
  out = torch.empty((n_img, cout, h, w), dtype=torch.float32, device=dev, memory_format=torch.channels_last)
  dil = (ctypes.c_int * groups)(*[int(d) for d in dilations])
  check(lib().spml_conv_tap_gather_f32(_ptr_any(z), _dp(bias), _ptr_any(out), n_img, h, w, cout, groups,
                                       ctypes.cast(dil, c_void_p), stream_ptr()), 'spml_conv_tap_gather_f32')
  return out


def hl8_weight_set(weights):
  """[(forward operand, data-gradient operand)] of up to four conv weights [Cout, Cin, kh, kw] in two
  launches (one unit's weights); every weight has its own bound / scale."""
  n = len(weights)
  dev = weights[0].device
  wl = [wt.detach().contiguous(memory_format=torch.channels_last) for wt in weights]
  bounds = torch.empty((4,), dtype=torch.float32, device=dev)
  shapes = [(wt.shape[0], wt.shape[1], wt.shape[2] * wt.shape[3]) for wt in wl]
  fwd = [torch.empty((co * ci * t * 4,), dtype=torch.uint8, device=dev) for co, ci, t in shapes]
  tr = [torch.empty((co * ci * t * 4,), dtype=torch.uint8, device=dev) for co, ci, t in shapes]
  pv, iv = ctypes.c_void_p * n, ctypes.c_int * n
  check(lib().spml_hl8_weight_set_f32(
      pv(*[wt.data_ptr() for wt in wl]), iv(*[sh[0] for sh in shapes]), iv(*[sh[1] for sh in shapes]),
      iv(*[sh[2] for sh in shapes]), n, _dp(bounds), pv(*[t.data_ptr() for t in fwd]),
      pv(*[t.data_ptr() for t in tr]), stream_ptr()), 'spml_hl8_weight_set_f32')
  out = []
  for i, (co, ci, t) in enumerate(shapes):
    b = bounds[i:i + 1]
    out.append((Hl8(fwd[i], b, co, t * ci), Hl8(tr[i], b, ci, t * co)))
  return out


def conv_hl8_affine(a, b, bias, n_img, h, w, taps, dilation=1, addend=None, relu=True, want_hl8=True):
  """Inference: act(conv(a, b) + bias [+ addend]) -> (out fp32 channels-last, Hl8 of it or None)."""
  k, n, out, operands = _conv_operands('conv_hl8_affine', a, b, n_img, h, w, taps)
  bound = _f32(1, out.device) if want_hl8 else None
  check(lib().spml_conv_hl8_affine_f32(*operands, ptr(bias, torch.float32), _ptr_any(addend, True), int(bool(relu)),
                                       _ptr_any(out), _dp(bound), n_img, h, w, k, n, taps, dilation, stream_ptr()),
        'spml_conv_hl8_affine_f32')
  return out, (hl8_from_f32(out, bound=bound) if want_hl8 else None)


# ---------------------------------------------------------------------------
# softmax head: cross-entropy of bilinearly up-sampled logits
def upsample_ce_supported(c):
  return bool(lib().spml_upsample_ce_supported(int(c)))


def upsample_ce_bwd_path_name(n, c, h, w, hh, ww):
  """Kernel the backward launches for [n, c, h, w] logits and [n, hh, ww] labels: 'tiled' or 'gather' (a pure host
  function of the library, the launch's own expression)."""
  return lib().spml_upsample_ce_bwd_path_name(int(n), int(c), int(h), int(w), int(hh), int(ww)).decode()


def upsample_ce_fwd(logits_nhwc, labels, ignore_index):
  """logits_nhwc fp32 [N, h, w, C] contiguous, labels int64 [N, H, W] -> (result [3] = sum, count, mean;
  lse [N, H, W])."""
  n, h, w, c = logits_nhwc.shape
  hh, ww = labels.shape[-2:]
  lse = torch.empty((n, hh, ww), dtype=torch.float32, device=logits_nhwc.device)
  result = torch.empty((3,), dtype=torch.float32, device=logits_nhwc.device)
  ws = workspace(lib().spml_upsample_ce_workspace_bytes(n, hh, ww), logits_nhwc.device)
  check(lib().spml_upsample_ce_fwd_f32(ptr(logits_nhwc, torch.float32), ptr(labels, torch.int64), n, c, h, w, hh, ww,
                                       int(ignore_index), ptr(lse), ptr(result), ptr(ws), ws.numel(), stream_ptr()),
        'spml_upsample_ce_fwd_f32')
  return result, lse


def upsample_ce_bwd(logits_nhwc, labels, lse, ignore_index, scale):
  """-> d_logits [N, h, w, C] = scale[0] * d(sum of the pixel losses) / d logits."""
  n, h, w, c = logits_nhwc.shape
  hh, ww = labels.shape[-2:]
  d = torch.empty_like(logits_nhwc)
  check(lib().spml_upsample_ce_bwd_f32(ptr(logits_nhwc, torch.float32), ptr(labels, torch.int64),
                                       ptr(lse, torch.float32), n, c, h, w, hh, ww, int(ignore_index),
                                       ptr(scale, torch.float32), ptr(d), stream_ptr()), 'spml_upsample_ce_bwd_f32')
  return d


# ---------------------------------------------------------------------------
# dense CRF refinement (csrc/dense_crf.hip)
MAX_DENSE_CRF_CLASSES = 64
MAX_DENSE_CRF_SIDE = 2048


def dense_crf_path_name(h, w, ncls, pos_xy_std):
  """Route a dense-CRF call of this shape takes: 'pairs_mfma_f16x2_c<32|64>+separable_r<R>' or 'unsupported' (a pure
  host function of the library)."""
  return lib().spml_dense_crf_path_name(int(h), int(w), int(ncls), float(pos_xy_std)).decode()


def dense_crf_workspace(h, w, ncls, device):
  nbytes = lib().spml_dense_crf_workspace_bytes(int(h), int(w), int(ncls))
  if nbytes == 0:
    raise SpmlHipError('the dense CRF takes one image of at most %d x %d pixels and %d classes (got %d x %d, %d classes)'
                       % (MAX_DENSE_CRF_SIDE, MAX_DENSE_CRF_SIDE, MAX_DENSE_CRF_CLASSES, h, w, ncls))
  return workspace(nbytes, device)


def dense_crf_prepare(image, pos_xy_std, bi_xy_std, bi_rgb_std, ws):
  """image uint8 [h, w, 3] -> the pair-exponent operands and both norms inside `ws` (dense_crf_workspace of any class
  count): once per image and set of standard deviations."""
  if image.dim() != 3 or image.shape[2] != 3:
    raise SpmlHipError('dense_crf_prepare: expected a uint8 [h, w, 3] image')
  h, w = int(image.shape[0]), int(image.shape[1])
  check(lib().spml_dense_crf_prepare_u8(ptr(image, torch.uint8), h, w, float(pos_xy_std), float(bi_xy_std),
                                        float(bi_rgb_std), ptr(ws), ws.numel(), stream_ptr()),
        'spml_dense_crf_prepare_u8')


def dense_crf_infer(probmap, iter_max, pos_w, bi_w, ws, want_labels=True):
  """probmap fp32 [ncls, h, w] and a prepared `ws` -> (Q fp32 [ncls, h, w], arg-max int64 [h, w] or None)."""
  if probmap.dim() != 3:
    raise SpmlHipError('dense_crf_infer: expected a [ncls, h, w] probability map')
  ncls, h, w = (int(v) for v in probmap.shape)
  q = torch.empty_like(probmap)
  labels = torch.empty((h, w), dtype=torch.int64, device=probmap.device) if want_labels else None
  check(lib().spml_dense_crf_infer_f32(ptr(probmap, torch.float32), ncls, h, w, int(iter_max), float(pos_w), float(bi_w),
                                       ptr(q), ptr(labels, torch.int64, True), ptr(ws), ws.numel(), stream_ptr()),
        'spml_dense_crf_infer_f32')
  return q, labels


def dense_crf_infer_upsampled(lowres, image_hw, iter_max, pos_w, bi_w, ws, want_labels=True, want_labels_before=True,
                              want_prob_up=False):
  """lowres fp32 [ncls, oh, ow], the image size (h, w) and a prepared `ws` -> (Q fp32 [ncls, h, w], arg-max int64 [h, w]
  or None, the arg-max of the up-sampled map before the CRF int64 [h, w] or None, the up-sampled map fp32 [ncls, h, w] or
  None): `dense_crf_infer` on the bilinear up-sampling of `lowres`, which the first launch forms in registers."""
  if lowres.dim() != 3:
    raise SpmlHipError('dense_crf_infer_upsampled: expected a [ncls, oh, ow] map')
  ncls, oh, ow = (int(v) for v in lowres.shape)
  h, w = (int(v) for v in image_hw)
  dev = lowres.device
  q = torch.empty((ncls, h, w), dtype=torch.float32, device=dev)
  labels = torch.empty((h, w), dtype=torch.int64, device=dev) if want_labels else None
  before = torch.empty((h, w), dtype=torch.int64, device=dev) if want_labels_before else None
  prob_up = torch.empty((ncls, h, w), dtype=torch.float32, device=dev) if want_prob_up else None
  check(lib().spml_dense_crf_infer_upsampled_f32(ptr(lowres, torch.float32), ncls, oh, ow, h, w, int(iter_max),
                                                 float(pos_w), float(bi_w), ptr(q), ptr(labels, torch.int64, True),
                                                 ptr(before, torch.int64, True), ptr(prob_up, torch.float32, True),
                                                 ptr(ws), ws.numel(), stream_ptr()),
        'spml_dense_crf_infer_upsampled_f32')
  return q, labels, before, prob_up


MAX_DENSE_CRF_VOTE_SEGMENTS = 4096     # the limit of spml_dense_crf_infer_votes_f32 (include/spml_hip.h)


def dense_crf_infer_votes(clu, topk, ncls, image_hw, iter_max, pos_w, bi_w, ws, want_labels=True, want_labels_before=True,
                          want_prob=False):
  """clu int64 `[h * w]` (or `[h, w]`), the dense segment id of every pixel; topk int64 `[m, k]`, the labels retrieved per
  segment; the class count, the image size (h, w) and a prepared `ws` -> (Q fp32 [ncls, h, w], arg-max int64 [h, w] or
  None, the arg-max of the votes before the CRF int64 [h, w] or None, the vote map fp32 [ncls, h, w] or None):
  `dense_crf_infer` on the vote map `one_hot(topk[clu]).sum(1) / k` (inference_crf.py:240-245), which the first launch
  gathers from a per-segment table instead of forming it.  All tensors contiguous, on the GPU."""
  for name, t in (('clu', clu), ('topk', topk), ('ws', ws)):
    if not torch.is_tensor(t) or not t.is_cuda:
      raise SpmlHipError('dense_crf_infer_votes: the HIP path needs GPU tensors (%s); there is no CPU fallback' % name)
  h, w = (int(v) for v in image_hw)
  ncls = int(ncls)
  if topk.dim() != 2 or h < 1 or w < 1 or clu.numel() != h * w:
    raise SpmlHipError('dense_crf_infer_votes: expected topk [m, k] and %d x %d segment ids' % (h, w))
  m, k = (int(v) for v in topk.shape)
  nbytes = lib().spml_dense_crf_votes_workspace_bytes(m, ncls)
  if nbytes == 0:
    raise SpmlHipError('dense_crf_infer_votes: %d segments x %d classes are outside the kernel (at most %d x %d)'
                       % (m, ncls, MAX_DENSE_CRF_VOTE_SEGMENTS, MAX_DENSE_CRF_CLASSES))
  dev = clu.device
  table = workspace(nbytes, dev)
  q = torch.empty((ncls, h, w), dtype=torch.float32, device=dev)
  labels = torch.empty((h, w), dtype=torch.int64, device=dev) if want_labels else None
  before = torch.empty((h, w), dtype=torch.int64, device=dev) if want_labels_before else None
  prob = torch.empty((ncls, h, w), dtype=torch.float32, device=dev) if want_prob else None
  check(lib().spml_dense_crf_infer_votes_f32(ptr(clu, torch.int64), ptr(topk, torch.int64), m, k, ncls, h, w,
                                             int(iter_max), float(pos_w), float(bi_w), ptr(q),
                                             ptr(labels, torch.int64, True), ptr(before, torch.int64, True),
                                             ptr(prob, torch.float32, True), ptr(table), table.numel(), ptr(ws),
                                             ws.numel(), stream_ptr()),
        'spml_dense_crf_infer_votes_f32')
  return q, labels, before, prob


# ---------------------------------------------------------------------------
# DensePose pseudo labels: class maps from propagated segment tags (csrc/segment_cam.hip)
MAX_SEGMENT_TAG_CAM_CLASSES = 64       # the limits of spml_segment_tag_cam_f32 (include/spml_hip.h)
MAX_SEGMENT_TAG_CAM_SEGMENTS = 4096


def segment_tag_cam_path_name(n, s, ncls):
  """Count kernel a call with these sizes takes (a pure function of the library): 'lds_table', 'global_table' or, outside
  the limits, 'unsupported'."""
  return lib().spml_segment_tag_cam_path_name(int(n), int(s), int(ncls)).decode()


def segment_tag_cam(nn_index, nn_value, proto_label, threshold, cluster_index, num_segments, ncls, half_hw, out_hw,
                    want_tables=False):
  """acc fp32 `[ncls, oh, ow]`: pseudo_denseposerw_crf.py:159-182 on `nn_index` int64 / `nn_value` fp32 `[N]` (what
  `topk_affinity(k = 1)` returns per pixel of the `half_hw` map, any shape with N = h2 * w2 entries), `proto_label` int64
  `[M]` and `cluster_index` int64 `[N]` (dense segment ids in `[0, num_segments)`): a pixel's class is
  `proto_label[nn_index]` (none where `nn_value < threshold` or the label is outside `[0, ncls)`), the classes are counted
  per segment, every row divided by its sum (zeros for a row without a count), and the map of rows `probs[cluster_index]`
  resampled bilinearly from `half_hw` to `out_hw`.  An index or id outside its range counts nowhere.  All tensors on the
  GPU (made contiguous here); no host read.  want_tables: -> (acc, counts int32 `[S, ncls]`, probs fp32 `[S, ncls]`)."""
  (h2, w2), (oh, ow) = (int(v) for v in half_hw), (int(v) for v in out_hw)
  s, ncls = int(num_segments), int(ncls)
  tensors = (('nn_index', nn_index, torch.int64), ('nn_value', nn_value, torch.float32),
             ('proto_label', proto_label, torch.int64), ('cluster_index', cluster_index, torch.int64))
  for name, t, dtype in tensors:
    if not torch.is_tensor(t) or not t.is_cuda:
      raise SpmlHipError('segment_tag_cam: the HIP path needs GPU tensors (%s on %s); there is no CPU fallback'
                         % (name, getattr(t, 'device', type(t).__name__)))
    if t.dtype != dtype:
      raise SpmlHipError('segment_tag_cam: %s must be %s (got %s)' % (name, dtype, t.dtype))
  if h2 < 1 or w2 < 1 or oh < 1 or ow < 1:
    raise SpmlHipError('segment_tag_cam: the maps need at least one pixel (got %r -> %r)' % ((h2, w2), (oh, ow)))
  n = h2 * w2
  for name, t, _ in tensors:
    if name != 'proto_label' and t.numel() != n:
      raise SpmlHipError('segment_tag_cam: %s holds %d entries for a %d x %d map' % (name, t.numel(), h2, w2))
  if proto_label.numel() < 1 or s < 1 or ncls < 1:
    raise SpmlHipError('segment_tag_cam: needs at least one prototype, one segment and one class (got %d, %d, %d)'
                       % (proto_label.numel(), s, ncls))
  nbytes = lib().spml_segment_tag_cam_workspace_bytes(s, ncls)
  if nbytes == 0:
    raise SpmlHipError('segment_tag_cam: %d segments x %d classes are outside the kernel (at most %d x %d)'
                       % (s, ncls, MAX_SEGMENT_TAG_CAM_SEGMENTS, MAX_SEGMENT_TAG_CAM_CLASSES))
  nn_index, nn_value, proto_label, cluster_index = (t.reshape(-1).contiguous() for _, t, _ in tensors)
  dev = cluster_index.device
  acc = torch.empty((ncls, oh, ow), dtype=torch.float32, device=dev)
  counts = torch.empty((s, ncls), dtype=torch.int32, device=dev) if want_tables else None
  probs = torch.empty((s, ncls), dtype=torch.float32, device=dev) if want_tables else None
  ws = workspace(nbytes, dev)
  check(lib().spml_segment_tag_cam_f32(ptr(nn_index, torch.int64), ptr(nn_value, torch.float32),
                                       ptr(proto_label, torch.int64), proto_label.numel(), float(threshold),
                                       ptr(cluster_index, torch.int64), s, ncls, h2, w2, oh, ow, ptr(acc),
                                       ptr(counts, torch.int32, True), ptr(probs, torch.float32, True), ptr(ws),
                                       ws.numel(), stream_ptr()), 'spml_segment_tag_cam_f32')
  return (acc, counts, probs) if want_tables else acc


# ---------------------------------------------------------------------------
# Training batches from decoded files: the fused augmentation launch (csrc/augment.hip)
def _augment_params_dtype():
  import numpy as np
  return np.dtype([('image_off', '<i8'), ('sem_off', '<i8'), ('inst_off', '<i8'), ('h', '<i4'), ('w', '<i4'),
                   ('new_h', '<i4'), ('new_w', '<i4'), ('start_h', '<i4'), ('start_w', '<i4'), ('flip', '<i4'),
                   ('gray', '<i4'), ('blur', '<i4'), ('reserved0', '<i4'), ('weights', '<f4', (25,)),
                   ('reserved1', '<f4')])


AUGMENT_PARAMS = _augment_params_dtype()      # spml_augment_params of include/spml_hip.h, field for field (168 bytes)


def _augment_records(params):
  """(host pointer, count) of a C-contiguous array of AUGMENT_PARAMS records whose size the library agrees with."""
  import numpy as np
  if not isinstance(params, np.ndarray) or params.dtype != AUGMENT_PARAMS or not params.flags['C_CONTIGUOUS']:
    raise SpmlHipError('augment: the records must be a contiguous numpy array of _ffi.AUGMENT_PARAMS')
  if lib().spml_augment_params_bytes() != AUGMENT_PARAMS.itemsize:
    raise SpmlHipError('augment: spml_augment_params is %d bytes in the library, %d here'
                       % (lib().spml_augment_params_bytes(), AUGMENT_PARAMS.itemsize))
  return c_void_p(params.ctypes.data), int(params.size)


def augment_path_name(record, packed_bytes, size):
  """'plain', 'blur' or 'unsupported' for one record (a host function of the library: the expression its launch
  evaluates for that record)."""
  host, n = _augment_records(record.reshape(1) if getattr(record, 'ndim', 1) == 0 else record)
  if n != 1:
    raise SpmlHipError('augment_path_name takes one record')
  return lib().spml_augment_path_name(host, int(packed_bytes), int(size[0]), int(size[1])).decode()


def _augment_params_dev(params_dev, n):
  if params_dev.dtype != torch.uint8 or params_dev.numel() != n * AUGMENT_PARAMS.itemsize:
    raise SpmlHipError('augment: params_dev must hold the %d records as %d bytes of uint8' % (n, n * AUGMENT_PARAMS.itemsize))
  return ptr(params_dev, torch.uint8)


def augment_batch(packed, params, params_dev, mean, std, remap, size, out=None):
  """One launch: `packed` uint8 (device; raw RGB + label planes) and `params` (host records; `params_dev` the same
  bytes on the device) -> image fp32 `[B, 3, S_h, S_w]`, semantic_label, instance_label int64 `[B, S_h, S_w]`.
  `out`: the three tensors to write into."""
  host, n = _augment_records(params)
  s_h, s_w = int(size[0]), int(size[1])
  dev_ptr = _augment_params_dev(params_dev, n)
  if out is None:
    dev = packed.device
    out = (torch.empty((n, 3, s_h, s_w), dtype=torch.float32, device=dev),
           torch.empty((n, s_h, s_w), dtype=torch.int64, device=dev),
           torch.empty((n, s_h, s_w), dtype=torch.int64, device=dev))
  image, sem, inst = out
  if tuple(image.shape) != (n, 3, s_h, s_w) or tuple(sem.shape) != (n, s_h, s_w) or tuple(inst.shape) != (n, s_h, s_w):
    raise SpmlHipError('augment_batch: outputs do not have the shapes of %d images at %d x %d' % (n, s_h, s_w))
  if mean.numel() != 3 or std.numel() != 3 or remap.numel() != 256:
    raise SpmlHipError('augment_batch: mean and std hold 3 values, the remap table 256')
  check(lib().spml_augment_batch_u8(ptr(packed, torch.uint8), packed.numel(), host, dev_ptr, n, ptr(mean, torch.float32),
                                    ptr(std, torch.float32), ptr(remap, torch.uint8), s_h, s_w,
                                    ptr(image, torch.float32), ptr(sem, torch.int64), ptr(inst, torch.int64),
                                    stream_ptr()), 'spml_augment_batch_u8')
  return image, sem, inst


def augment_tags(packed, params, params_dev, out=None):
  """semantic_tag int64 `[B, 256]`: the multi-hot of the values in the un-augmented semantic planes of `packed`."""
  host, n = _augment_records(params)
  dev_ptr = _augment_params_dev(params_dev, n)
  if out is None:
    out = torch.empty((n, 256), dtype=torch.int64, device=packed.device)
  if tuple(out.shape) != (n, 256):
    raise SpmlHipError('augment_tags: the output must be [%d, 256]' % n)
  check(lib().spml_augment_tags_u8(ptr(packed, torch.uint8), packed.numel(), host, dev_ptr, n, ptr(out, torch.int64),
                                   stream_ptr()), 'spml_augment_tags_u8')
  return out


# ---------------------------------------------------------------------------
# Inference from decoded files: the view pyramid and the label export (csrc/inference_io.hip)
def _view_params_dtype():
  import numpy as np
  return np.dtype([('image_off', '<i8'), ('label_off', '<i8'), ('new_h', '<i4'), ('new_w', '<i4'), ('pad_h', '<i4'),
                   ('pad_w', '<i4'), ('flip', '<i4'), ('reserved0', '<i4')])


VIEW_PARAMS = _view_params_dtype()            # spml_view_params of include/spml_hip.h, field for field (40 bytes)


def _view_records(params):
  """(host pointer, count) of a C-contiguous array of VIEW_PARAMS records whose size the library agrees with."""
  import numpy as np
  if not isinstance(params, np.ndarray) or params.dtype != VIEW_PARAMS or not params.flags['C_CONTIGUOUS']:
    raise SpmlHipError('image_views: the records must be a contiguous numpy array of _ffi.VIEW_PARAMS')
  if lib().spml_view_params_bytes() != VIEW_PARAMS.itemsize:
    raise SpmlHipError('image_views: spml_view_params is %d bytes in the library, %d here'
                       % (lib().spml_view_params_bytes(), VIEW_PARAMS.itemsize))
  return c_void_p(params.ctypes.data), int(params.size)


def image_views_path_name(params, source_hw, image_bytes, label_bytes=0, with_labels=False):
  """'views', 'views+labels' or 'unsupported' for the records of one image (a host function of the library: the
  expression its entry evaluates before the launch)."""
  host, n = _view_records(params)
  return lib().spml_image_views_path_name(host, n, int(source_hw[0]), int(source_hw[1]), int(image_bytes),
                                          int(label_bytes), int(bool(with_labels))).decode()


def image_views(rgb, semantic, params, params_dev, mean, std, images, labels=None):
  """One launch: `rgb` uint8 `[h, w, 3]` (+ `semantic` uint8 `[h, w]`), both on the device, and `params` (host records;
  `params_dev` the same bytes on the device) -> every view into `images` (fp32, flat) at its `image_off` and, with a
  label, into `labels` (int64, flat) at its `label_off`."""
  host, n = _view_records(params)
  if rgb.dim() != 3 or rgb.shape[2] != 3:
    raise SpmlHipError('image_views: rgb must be uint8 [h, w, 3]')
  h, w = int(rgb.shape[0]), int(rgb.shape[1])
  if (semantic is None) != (labels is None):
    raise SpmlHipError('image_views: the label buffer goes with the semantic plane')
  if semantic is not None and tuple(semantic.shape) != (h, w):
    raise SpmlHipError('image_views: the semantic plane must be uint8 [%d, %d]' % (h, w))
  if params_dev.dtype != torch.uint8 or params_dev.numel() != n * VIEW_PARAMS.itemsize:
    raise SpmlHipError('image_views: params_dev must hold the %d records as %d bytes of uint8' % (n, n * VIEW_PARAMS.itemsize))
  if mean.numel() != 3 or std.numel() != 3:
    raise SpmlHipError('image_views: mean and std hold 3 values')
  check(lib().spml_image_views_u8(ptr(rgb, torch.uint8), ptr(semantic, torch.uint8, allow_none=True), h, w,
                                  ptr(mean, torch.float32), ptr(std, torch.float32), host, ptr(params_dev, torch.uint8), n,
                                  ptr(images, torch.float32), images.numel() * 4, ptr(labels, torch.int64, allow_none=True),
                                  0 if labels is None else labels.numel() * 8, stream_ptr()), 'spml_image_views_u8')
  return images, labels


def label_export_path_name(pred_hw, valid_hw, out_hw):
  return lib().spml_label_export_path_name(int(pred_hw[0]), int(pred_hw[1]), int(valid_hw[0]), int(valid_hw[1]),
                                           int(out_hw[0]), int(out_hw[1])).decode()


def label_export(prediction, valid_hw, out_hw, color_map, out=None):
  """One launch: `prediction` int64 `[pred_h, pred_w]`, its valid top-left rectangle, `color_map` uint8 `[256, 3]`
  -> (gray uint8 `[out_h, out_w]`, rgb uint8 `[out_h, out_w, 3]`).  `out`: the two tensors to write into."""
  if prediction.dim() != 2:
    raise SpmlHipError('label_export: the prediction must be int64 [pred_h, pred_w]')
  if tuple(color_map.shape) != (256, 3):
    raise SpmlHipError('label_export: the colour map must be uint8 [256, 3]')
  oh, ow = int(out_hw[0]), int(out_hw[1])
  if out is None:
    if oh < 1 or ow < 1:
      raise SpmlHipError('label_export: an output of %d x %d' % (oh, ow))
    out = (torch.empty((oh, ow), dtype=torch.uint8, device=prediction.device),
           torch.empty((oh, ow, 3), dtype=torch.uint8, device=prediction.device))
  gray, rgb = out
  if tuple(gray.shape) != (oh, ow) or tuple(rgb.shape) != (oh, ow, 3):
    raise SpmlHipError('label_export: outputs do not have the shapes of a %d x %d map' % (oh, ow))
  check(lib().spml_label_export_u8(ptr(prediction, torch.int64), int(prediction.shape[0]), int(prediction.shape[1]),
                                   int(valid_hw[0]), int(valid_hw[1]), oh, ow, ptr(color_map, torch.uint8),
                                   ptr(gray, torch.uint8), ptr(rgb, torch.uint8), stream_ptr()), 'spml_label_export_u8')
  return gray, rgb


MAX_EXPORT_SCORE_CLASSES = 256         # the limit of spml_label_export_scored_u8 (include/spml_hip.h)


def crf_guide_path_name(source_hw, out_hw=None):
  """'guide_table', 'guide_resized' or 'unsupported' (a host function of the library)."""
  out_hw = source_hw if out_hw is None else out_hw
  return lib().spml_crf_guide_path_name(int(source_hw[0]), int(source_hw[1]), int(out_hw[0]), int(out_hw[1])).decode()


def crf_guide(rgb, mean, std, pixel_means, pixel_stds, out_hw=None, out=None):
  """One launch: `rgb` uint8 `[h, w, 3]` on the device -> the dense CRF's guide uint8 `[new_h, new_w, 3]` (`out_hw`; the
  source's own size when None).  `mean` / `std`: the fp32 `[3]` device tensors of `image_views`; `pixel_means` /
  `pixel_stds`: the same statistics as Python numbers (they go to the library as doubles)."""
  import ctypes
  if rgb.dim() != 3 or rgb.shape[2] != 3:
    raise SpmlHipError('crf_guide: rgb must be uint8 [h, w, 3]')
  if mean.numel() != 3 or std.numel() != 3 or len(pixel_means) != 3 or len(pixel_stds) != 3:
    raise SpmlHipError('crf_guide: mean and std hold 3 values')
  h, w = int(rgb.shape[0]), int(rgb.shape[1])
  new_h, new_w = (h, w) if out_hw is None else (int(out_hw[0]), int(out_hw[1]))
  if out is None:
    if new_h < 1 or new_w < 1:
      raise SpmlHipError('crf_guide: an output of %d x %d' % (new_h, new_w))
    out = torch.empty((new_h, new_w, 3), dtype=torch.uint8, device=rgb.device)
  elif tuple(out.shape) != (new_h, new_w, 3):
    raise SpmlHipError('crf_guide: the output must be uint8 [%d, %d, 3]' % (new_h, new_w))
  mean64 = (ctypes.c_double * 3)(*(float(v) for v in pixel_means))
  std64 = (ctypes.c_double * 3)(*(float(v) for v in pixel_stds))
  check(lib().spml_crf_guide_u8(ptr(rgb, torch.uint8), h, w, ptr(mean, torch.float32), ptr(std, torch.float32), mean64,
                                std64, new_h, new_w, ptr(out, torch.uint8), stream_ptr()), 'spml_crf_guide_u8')
  return out


def export_scores_bytes(ncls):
  return int(lib().spml_export_scores_bytes(int(ncls)))


def label_export_scored(refined, before, valid_hw, out_hw, color_map, truth, ncls, scores, out=None):
  """One launch: `label_export` of `refined` + the same resampling of `before` (int64 `[pred_h, pred_w]` or None), both
  counted against `truth` (uint8 `[out_h, out_w]` or None) INTO `scores` (int64 `[2 * 3 * ncls + 1]`: the two
  `[3, ncls]` tables of `iou_counts`, then the number of output pixels the two maps differ at).
  -> (gray uint8 `[out_h, out_w]`, rgb uint8 `[out_h, out_w, 3]`)."""
  if refined.dim() != 2 or (before is not None and tuple(before.shape) != tuple(refined.shape)):
    raise SpmlHipError('label_export_scored: the two predictions must be int64 [pred_h, pred_w]')
  if tuple(color_map.shape) != (256, 3):
    raise SpmlHipError('label_export_scored: the colour map must be uint8 [256, 3]')
  oh, ow = int(out_hw[0]), int(out_hw[1])
  if truth is not None and tuple(truth.shape) != (oh, ow):
    raise SpmlHipError('label_export_scored: the ground truth must be uint8 [%d, %d]' % (oh, ow))
  nbytes = export_scores_bytes(ncls)
  if nbytes and scores.numel() * 8 != nbytes:
    raise SpmlHipError('label_export_scored: scores must hold 2 * 3 * %d + 1 int64 values' % int(ncls))
  if out is None:
    if oh < 1 or ow < 1:
      raise SpmlHipError('label_export_scored: an output of %d x %d' % (oh, ow))
    out = (torch.empty((oh, ow), dtype=torch.uint8, device=refined.device),
           torch.empty((oh, ow, 3), dtype=torch.uint8, device=refined.device))
  gray, rgb = out
  if tuple(gray.shape) != (oh, ow) or tuple(rgb.shape) != (oh, ow, 3):
    raise SpmlHipError('label_export_scored: outputs do not have the shapes of a %d x %d map' % (oh, ow))
  check(lib().spml_label_export_scored_u8(
      ptr(refined, torch.int64), ptr(before, torch.int64, allow_none=True), int(refined.shape[0]), int(refined.shape[1]),
      int(valid_hw[0]), int(valid_hw[1]), oh, ow, ptr(color_map, torch.uint8), ptr(truth, torch.uint8, allow_none=True),
      int(ncls), ptr(gray, torch.uint8), ptr(rgb, torch.uint8), ptr(scores, torch.int64), stream_ptr()),
        'spml_label_export_scored_u8')
  return gray, rgb


# ---------------------------------------------------------------------------
# Scoring label files against ground truth, a batch of decoded files per call (csrc/score_batch.hip)
MAX_SCORE_FILES = 256                  # the limits of spml_score_batch_u8 (include/spml_hip.h)
MAX_SCORE_CLASSES = 64
SCORE_PLANE_ALIGN = 16                 # plane offsets and padded plane sizes are multiples of this


def _score_params_dtype():
  import numpy as np
  return np.dtype([('pred_off', '<i8'), ('gt_off', '<i8'), ('inst_off', '<i8'), ('n', '<i8')])


SCORE_PARAMS = _score_params_dtype()          # spml_score_params of include/spml_hip.h, field for field (32 bytes)


def _score_records(records):
  """(host pointer, count) of a C-contiguous array of SCORE_PARAMS records whose size the library agrees with."""
  import numpy as np
  if not isinstance(records, np.ndarray) or records.dtype != SCORE_PARAMS or not records.flags['C_CONTIGUOUS']:
    raise SpmlHipError('score_batch: the records must be a contiguous numpy array of _ffi.SCORE_PARAMS')
  if lib().spml_score_params_bytes() != SCORE_PARAMS.itemsize:
    raise SpmlHipError('score_batch: spml_score_params is %d bytes in the library, %d here'
                       % (lib().spml_score_params_bytes(), SCORE_PARAMS.itemsize))
  return c_void_p(records.ctypes.data), int(records.size)


def score_batch_path_name(records, packed_bytes, ncls):
  """'lds_table', 'global_table' or 'unsupported' for the records of one batch (a host function of the library: the
  expression its entry evaluates before the launch)."""
  host, n = _score_records(records)
  return lib().spml_score_batch_path_name(host, n, int(packed_bytes), int(ncls)).decode()


def score_batch(packed, records, ncls, params_dev=None, out=None):
  """stats int64 `[B, 4, ncls]` (TP+FN, TP+FP, TP, instances per class) of the B files whose uint8 planes lie in
  `packed` (uint8, on the device) where `records` (host, SCORE_PARAMS) say.  `params_dev`: the same records as bytes of
  uint8 on the device, for a caller that uploaded them with the planes; copied up here otherwise.  No host read."""
  host, n = _score_records(records)
  ncls = int(ncls)
  ptr(packed, torch.uint8)                                   # (CPU tensors are refused before anything is allocated)
  if params_dev is None:
    params_dev = torch.from_numpy(records.view('u1').reshape(-1).copy()).to(packed.device)
  if params_dev.dtype != torch.uint8 or params_dev.numel() != n * SCORE_PARAMS.itemsize:
    raise SpmlHipError('score_batch: params_dev must hold the %d records as %d bytes of uint8' % (n, n * SCORE_PARAMS.itemsize))
  if out is None:
    if n < 1 or ncls < 1:
      raise SpmlHipError('score_batch: needs at least one file and one class (got %d, %d)' % (n, ncls))
    out = torch.empty((n, 4, ncls), dtype=torch.int64, device=packed.device)
  if tuple(out.shape) != (n, 4, ncls):
    raise SpmlHipError('score_batch: the output must be [%d, 4, %d]' % (n, ncls))
  ws = workspace(lib().spml_score_batch_workspace_bytes(n, ncls), packed.device)
  check(lib().spml_score_batch_u8(ptr(packed, torch.uint8), packed.numel(), host, ptr(params_dev, torch.uint8), n, ncls,
                                  ptr(out, torch.int64), ptr(ws), ws.numel(), stream_ptr()), 'spml_score_batch_u8')
  return out


# ---------------------------------------------------------------------------
# The picture of a training summary (csrc/train_summary.hip)
def pca_path_name(c, pixel_stride, channel_stride):
  """'gram_mfma_f32_c32', 'gram_mfma_f32_c64', the same with '_nchw', or 'unsupported' (a host function of the library:
  the expression its entries evaluate before the launch)."""
  return lib().spml_pca_path_name(int(c), int(pixel_stride), int(channel_stride)).decode()


def embedding_strides(emb):
  """(pixel_stride, channel_stride) in elements of a dense fp32 `[N, C, H, W]` GPU tensor: `(C, 1)` for channels-last
  storage, `(1, H * W)` for NCHW-contiguous."""
  _ptr_any(emb)
  if emb.dim() != 4:
    raise SpmlHipError('the embedding must be [N, C, H, W] (got %s)' % (tuple(emb.shape),))
  n, c, h, w = emb.shape
  if emb.is_contiguous(memory_format=torch.channels_last):
    return c, 1
  if emb.is_contiguous():
    return 1, h * w
  raise SpmlHipError('the embedding must be channels-last or NCHW-contiguous')


def _summary_workspace(emb, ws):
  n, c, h, w = emb.shape
  need = lib().spml_train_summary_workspace_bytes(n, c, h, w)
  return workspace(need, emb.device) if ws is None else ws


def pca_moments(emb, ws=None):
  """mean fp64 `[C]` and covariance fp64 `[C, C]` (divided by P - 1) of the L2-normalised pixels of `emb`."""
  ps, cs = embedding_strides(emb)
  n, c, h, w = emb.shape
  ws = _summary_workspace(emb, ws)
  mean = torch.empty((c,), dtype=torch.float64, device=emb.device)
  cov = torch.empty((c, c), dtype=torch.float64, device=emb.device)
  check(lib().spml_pca_moments_f32(_ptr_any(emb), n, c, h, w, ps, cs, ptr(mean), ptr(cov), ptr(ws), ws.numel(),
                                   stream_ptr()), 'spml_pca_moments_f32')
  return mean, cov


def pca_project_minmax(emb, basis, ws=None):
  """proj fp32 `[N, H, W, 3]` = normalised pixel . `basis` (fp32 `[C, 3]`, un-centred) and minmax fp32 `[N, 3, 2]`, the
  (minimum, maximum) of proj per image and channel."""
  ps, cs = embedding_strides(emb)
  n, c, h, w = emb.shape
  if tuple(basis.shape) != (c, 3):
    raise SpmlHipError('pca_project_minmax: the basis must be fp32 [%d, 3]' % c)
  ws = _summary_workspace(emb, ws)
  proj = torch.empty((n, h, w, 3), dtype=torch.float32, device=emb.device)
  minmax = torch.empty((n, 3, 2), dtype=torch.float32, device=emb.device)
  check(lib().spml_pca_project_minmax_f32(_ptr_any(emb), n, c, h, w, ps, cs, ptr(basis, torch.float32), ptr(proj),
                                          ptr(minmax), ptr(ws), ws.numel(), stream_ptr()), 'spml_pca_project_minmax_f32')
  return proj, minmax


def summary_panels(semantic, instance, proj, minmax, color_map, out=None):
  """One launch: the label maps int64 `[N, Hl, Wl]`, proj fp32 `[N, h, w, 3]` and minmax fp32 `[N, 3, 2]` of
  `pca_project_minmax`, `color_map` uint8 `[256, 3]` -> the picture uint8 `[3, Htot, Wtot]` of
  `vis.summary_grid_shape(N, h, w)`.  Without label maps (both None): the embedding panel alone, uint8 `[N, 3, h, w]`."""
  from .utils.general.vis import summary_grid_padding, summary_grid_shape
  if proj.dim() != 4 or proj.shape[3] != 3:
    raise SpmlHipError('summary_panels: proj must be fp32 [N, h, w, 3]')
  n, h, w = int(proj.shape[0]), int(proj.shape[1]), int(proj.shape[2])
  if tuple(minmax.shape) != (n, 3, 2):
    raise SpmlHipError('summary_panels: minmax must be fp32 [%d, 3, 2]' % n)
  if (semantic is None) != (instance is None):
    raise SpmlHipError('summary_panels: the two label maps go together')
  if semantic is None:
    shape, pad, hl, wl, out_h, out_w = (n, 3, h, w), 0, 0, 0, 0, 0
  else:
    if semantic.dim() != 3 or semantic.shape[0] != n or semantic.shape != instance.shape:
      raise SpmlHipError('summary_panels: the label maps must be int64 [%d, Hl, Wl], both of one size' % n)
    if tuple(color_map.shape) != (256, 3):
      raise SpmlHipError('summary_panels: the colour map must be uint8 [256, 3]')
    hl, wl = int(semantic.shape[1]), int(semantic.shape[2])
    out_h, out_w = summary_grid_shape(n, h, w)
    shape, pad = (3, out_h, out_w), summary_grid_padding(n)
  if out is None:
    out = torch.empty(shape, dtype=torch.uint8, device=proj.device)
  if tuple(out.shape) != shape:
    raise SpmlHipError('summary_panels: the output must be uint8 %s' % (shape,))
  check(lib().spml_summary_panels_u8(ptr(semantic, torch.int64, allow_none=True), ptr(instance, torch.int64, allow_none=True),
                                     n, hl, wl, ptr(proj, torch.float32), ptr(minmax, torch.float32), h, w,
                                     ptr(color_map, torch.uint8, allow_none=semantic is None), pad, out_h, out_w,
                                     ptr(out, torch.uint8), stream_ptr()), 'spml_summary_panels_u8')
  return out


# ---------------------------------------------------------------------------
# CAM ingest (csrc/cam_ingest.hip)
MAX_CAM_CLASSES = 256                  # the limit of spml_cam_ingest_f32 (include/spml_hip.h)


def cam_ingest_path_name(k, h, w, ncls):
  """'cam_ingest' or 'unsupported' (a host function of the library)."""
  return lib().spml_cam_ingest_path_name(int(k), int(h), int(w), int(ncls)).decode()


def cam_ingest(planes, classes, hw, ncls, alpha, out=None):
  """One launch: the `K` planes a CAM file carries, fp32 `[K, h, w]` on the device (None or `[0, h, w]` for a file
  without entries), and `classes`, their `K` dict keys (class - 1) as host integers -> fp32 `[ncls, h // 8, w // 8]`, the
  background row and the 1/8 bilinear reduction of pseudo_camrw_crf.py:108-111,151-152.  The keys are checked by the
  library on the host (range, duplicates) before anything is launched."""
  import ctypes
  h, w = int(hw[0]), int(hw[1])
  keys = [int(c) for c in classes]
  k = len(keys)
  if planes is None:
    if k:
      raise SpmlHipError('cam_ingest: %d classes without planes' % k)
    device = torch.device('cuda', torch.cuda.current_device())
  else:
    if planes.dim() != 3 or tuple(planes.shape) != (k, h, w):
      raise SpmlHipError('cam_ingest: planes must be fp32 [%d, %d, %d], one per class key' % (k, h, w))
    device = planes.device
  oh, ow = h // 8, w // 8
  if out is None:
    if oh < 1 or ow < 1 or int(ncls) < 1:
      raise SpmlHipError('cam_ingest: no output for a %d x %d image and %d classes' % (h, w, int(ncls)))
    out = torch.empty((int(ncls), oh, ow), dtype=torch.float32, device=device)
  elif tuple(out.shape) != (int(ncls), oh, ow):
    raise SpmlHipError('cam_ingest: the output must be fp32 [%d, %d, %d]' % (int(ncls), oh, ow))
  keys_host = (ctypes.c_int * max(k, 1))(*keys)
  planes_ptr = ptr(planes, torch.float32, allow_none=True)            # (checked for an empty tensor too)
  check(lib().spml_cam_ingest_f32(planes_ptr if k else c_void_p(0), keys_host, k, h, w, int(ncls), int(alpha),
                                  ptr(out, torch.float32), stream_ptr()), 'spml_cam_ingest_f32')
  return out
