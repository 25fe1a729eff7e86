"""ctypes binding of libsnnhip.so (C ABI: include/snn_hip.h).  There is NO fallback: if the HIP
library is missing or a call fails, the product path raises."""
import ctypes as C
import os

from . import build as _build

c_f32p = C.POINTER(C.c_float)
c_u32p = C.POINTER(C.c_uint32)
c_u64p = C.POINTER(C.c_ulonglong)
c_stream = C.c_void_p

SNN_MAX_LEVELS = 8
SNN_MAX_STEPS = 32
FEAT_DTYPES = {"f32": 0, "f16": 1, "bf16": 2}          # SNN_FEAT_*
FEAT_NHWC = 16                                            # SNN_FEAT_NHWC: layout bit, OR-ed into a FEAT_DTYPES code (channels-last maps)
NO_TYPED_KERNEL = 1                                       # SNN_STATUS_NO_TYPED_KERNEL: nothing was enqueued; widen and call with "f32"
PRECISIONS = {"f32": 0, "bf16x3": 1, "mxfp6": 2, "f32_strict": 3, "bf16": 4}
CONV_ROUTES = {"sparse": 0, "dense": 1, "auto": 2}      # SNN_ROUTE_*
ROUTE_DEFAULT_CROSSOVER = 0.357                            # SNN_ROUTE_DEFAULT_CROSSOVER (tests/test_conv_route_cpu.py compares it with the header)
FC6_ROUTE_DEFAULT_CROSSOVER = 0.061                         # SNN_FC6_ROUTE_DEFAULT_CROSSOVER (tests/test_fc6_route_cpu.py compares it with the header)


class snn_params(C.Structure):
    _fields_ = [("dt_tau_mem", C.c_float), ("neg_dt_tau_syn", C.c_float), ("v_leak", C.c_float),
                ("v_reset", C.c_float), ("v_th_enc", C.c_float), ("v_th_lif", C.c_float),
                ("li_order", C.c_int32), ("precision", C.c_int32)]


class snn_rpn_level(C.Structure):
    _fields_ = [("feat", C.c_void_p), ("N", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("precision", C.c_int32)]


class snn_roi_level(C.Structure):
    _fields_ = [("feat", C.c_void_p), ("H", C.c_int32), ("W", C.c_int32), ("spatial_scale", C.c_float),
                ("reserved", C.c_int32)]


class snn_rpn_post_level(C.Structure):
    _fields_ = [("logits", C.c_void_p), ("deltas", C.c_void_p), ("H", C.c_int32), ("W", C.c_int32),
                ("stride_h", C.c_float), ("stride_w", C.c_float), ("base_anchors", (C.c_float * 4) * 16)]


PLANE_LAYOUTS = {"rows": 0, "split4": 1, "word_major": 2}   # SNN_PLANES_*


class snn_planes_view(C.Structure):
    _fields_ = [("offset_bytes", C.c_uint64), ("step_stride_words", C.c_uint64), ("rows", C.c_int64), ("words", C.c_int32),
                ("layout", C.c_int32), ("steps_formed", C.c_int32), ("reserved", C.c_int32)]


# every symbol include/snn_hip_debug.h declares (test plumbing of the same .so, not the drop-in boundary)
DEBUG_SYMBOLS = {
    "snn_debug_reload_knobs": (None, []),
    "snn_debug_encoder_thresholds": (C.c_int, [C.POINTER(snn_params), C.POINTER(C.c_float)]),
    "snn_debug_last_enc_mode": (C.c_int, []),
    "snn_debug_last_conv_path": (C.c_int, []),
    "snn_debug_last_fc6_path": (C.c_int, []),
    "snn_debug_last_det_planes": (None, [C.POINTER(C.c_uint64)]),
    "snn_debug_last_rpn_planes": (None, [C.POINTER(C.c_uint64)]),
    "snn_debug_tile_shape": (C.c_int, [C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32)]),
    "snn_debug_clock_probe": (C.c_int, [C.c_void_p, C.c_uint, c_stream]),
}

# every symbol include/snn_hip.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "snn_version": (C.c_int, []),
    "snn_last_error": (C.c_char_p, []),
    "snn_packed_gemm_elems": (C.c_size_t, [C.c_int, C.c_int]),
    "snn_packed_conv3x3_elems": (C.c_size_t, [C.c_int, C.c_int]),
    "snn_pack_conv3x3_weight": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, c_stream]),
    "snn_packed_linear_elems": (C.c_size_t, [C.c_int, C.c_int]),
    "snn_pack_linear_weight": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, c_stream]),
    "snn_packed_heads_elems": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "snn_pack_heads_weight": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, c_stream]),
    "snn_rpn_head_workspace_bytes": (C.c_size_t, [C.POINTER(snn_rpn_level), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "snn_rpn_head_forward": (C.c_int, [C.POINTER(snn_rpn_level), C.c_int, C.c_int, C.c_int, C.c_int,
                                       C.POINTER(snn_params), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, c_stream]),
    "snn_rpn_head_forward_stages": (C.c_int, [C.POINTER(snn_rpn_level), C.c_int, C.c_int, C.c_int, C.c_int,
                                              C.POINTER(snn_params), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int,
                                              c_stream]),
    "snn_det_head_workspace_bytes": (C.c_size_t, [C.c_int] * 7),
    "snn_det_head_forward": (C.c_int, [C.c_void_p] + [C.c_int] * 6 + [C.POINTER(snn_params)] +
                             [C.c_void_p] * 10 + [C.c_size_t, c_stream]),
    "snn_rpn_rates_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "snn_rpn_rates": (C.c_int, [C.POINTER(snn_rpn_level), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_void_p, C.c_size_t, c_stream]),
    "snn_det_rates": (C.c_int, [C.c_int] * 7 + [C.c_void_p] * 5 + [c_stream]),
    "snn_affine_act_nchw": (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 4 + [C.c_void_p, c_stream]),
    "snn_encode_nchw": (C.c_int, [C.c_void_p] + [C.c_int] * 5 + [C.POINTER(snn_params), C.c_void_p, C.c_size_t, c_stream]),
    "snn_encode_rows": (C.c_int, [C.c_void_p] + [C.c_int] * 3 + [C.POINTER(snn_params), C.c_void_p, C.c_size_t, c_stream]),
    "snn_conv3x3_lif": (C.c_int, [C.c_void_p, C.c_size_t] + [C.c_int] * 6 + [C.POINTER(snn_params), C.c_void_p,
                                  C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, c_stream]),
    "snn_spike_gemm": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, c_stream]),
    "snn_lif_scan": (C.c_int, [C.c_void_p] + [C.c_int] * 4 + [C.POINTER(snn_params), C.c_void_p, C.c_size_t,
                               C.c_void_p, c_stream]),
    "snn_li_heads": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                               C.POINTER(snn_params), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, c_stream]),
    "snn_nms_workspace_bytes": (C.c_size_t, [C.c_int]),
    "snn_rpn_proposals_candidates": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "snn_rpn_proposals_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "snn_rpn_proposals": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float,
                                    C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                    c_stream]),
    "snn_det_postprocess_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "snn_det_postprocess": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_float,
                                      C.c_float, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, c_stream]),
    # the static-shape path: per-image row counts read on the device
    "snn_roi_assign": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p,
                                 C.c_void_p, c_stream]),
    "snn_det_postprocess_padded": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                             C.c_float, C.c_float, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, c_stream]),
    "snn_pack_padded_detections": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                             c_stream]),
    "snn_det_exchange_payload": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                           c_stream]),
    "snn_nms_sorted": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_size_t, c_stream]),
    "snn_roi_align_encode": (C.c_int, [C.POINTER(snn_roi_level), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_int, C.c_int, C.POINTER(snn_params), C.c_void_p, C.c_size_t, C.c_void_p, c_stream]),
    "snn_det_head_forward_roialign": (C.c_int, [C.POINTER(snn_roi_level), C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                                C.c_void_p] + [C.c_int] * 5 + [C.POINTER(snn_params)] +
                                      [C.c_void_p] * 10 + [C.c_size_t, c_stream]),
    "snn_packed_bf16x3_elems": (C.c_size_t, [C.c_int, C.c_int]),
    "snn_packed_conv3x3_bf16x3_elems": (C.c_size_t, [C.c_int, C.c_int]),
    "snn_pack_conv3x3_weight_bf16x3": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, c_stream]),
    "snn_packed_linear_bf16x3_elems": (C.c_size_t, [C.c_int, C.c_int]),
    "snn_pack_linear_weight_bf16x3": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, c_stream]),
    "snn_packed_bf16_elems": (C.c_size_t, [C.c_int, C.c_int]),
    "snn_packed_conv3x3_bf16_elems": (C.c_size_t, [C.c_int, C.c_int]),
    "snn_pack_conv3x3_weight_bf16": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, c_stream]),
    "snn_packed_linear_bf16_elems": (C.c_size_t, [C.c_int, C.c_int]),
    "snn_pack_linear_weight_bf16": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, c_stream]),
    "snn_pack_linear_weight_bf16_perm": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, c_stream]),
    "snn_check_bf16x3_split": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, c_stream]),
    "snn_pack_linear_weight_bf16x3_perm": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, c_stream]),
    "snn_det_head_forward_k": (C.c_int, [C.c_void_p] + [C.c_int] * 6 + [C.POINTER(snn_params), C.c_void_p, C.c_int] +
                               [C.c_void_p] * 9 + [C.c_size_t, c_stream]),
    "snn_det_head_forward_roialign_k": (C.c_int, [C.POINTER(snn_roi_level), C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                                  C.c_void_p] + [C.c_int] * 5 + [C.POINTER(snn_params), C.c_void_p, C.c_int] +
                                        [C.c_void_p] * 9 + [C.c_size_t, c_stream]),
    "snn_li_heads_readouts": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                        C.POINTER(snn_params), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, c_stream]),
    "snn_rpn_head_forward_readouts": (C.c_int, [C.POINTER(snn_rpn_level), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                                C.POINTER(snn_params)] + [C.c_void_p] * 8 + [C.c_size_t, c_stream]),
    "snn_det_head_forward_readouts": (C.c_int, [C.c_void_p] + [C.c_int] * 5 + [C.c_void_p, C.c_int, C.POINTER(snn_params),
                                                C.c_void_p, C.c_int] + [C.c_void_p] * 9 + [C.c_size_t, c_stream]),
    "snn_det_head_forward_roialign_readouts": (C.c_int, [C.POINTER(snn_roi_level), C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                                         C.c_void_p] + [C.c_int] * 4 + [C.c_void_p, C.c_int, C.POINTER(snn_params),
                                                         C.c_void_p, C.c_int] + [C.c_void_p] * 9 + [C.c_size_t, c_stream]),
    "snn_packed_linear_mx_words": (C.c_size_t, [C.c_int, C.c_int]),
    "snn_packed_conv3x3_mx_words": (C.c_size_t, [C.c_int, C.c_int]),
    "snn_pack_linear_weight_mx": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, c_stream]),
    "snn_pack_conv3x3_weight_mx": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, c_stream]),
    "snn_spike_gemm_mx": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, c_stream]),
    "snn_spike_gemm_lif_mx": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_size_t, c_stream]),
    "snn_conv3x3_lif_mx": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_size_t, c_stream]),
    "snn_spike_conv3x3_mx": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                       C.c_void_p, C.c_int, c_stream]),
    "snn_spike_gemm_bf16x3": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, c_stream]),
    "snn_spike_gemm_lif_bf16x3": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_size_t, c_stream]),
    "snn_conv3x3_lif_bf16x3": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(snn_rpn_level), C.c_int, C.c_int, C.c_int,
                                         C.c_int, C.POINTER(snn_params), C.c_void_p, C.c_void_p, C.c_size_t, c_stream]),
    "snn_spike_conv3x3_bf16x3": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(snn_rpn_level), C.c_int, C.c_int, C.c_int,
                                           C.c_int, C.c_void_p, C.c_void_p, C.c_int, c_stream]),
    # the typed twins (half-precision features): the untyped signature with an int feat_dtype behind the feature argument
    "snn_rpn_head_forward_stages_typed": (C.c_int, [C.POINTER(snn_rpn_level), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                    C.POINTER(snn_params), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int,
                                                    c_stream]),
    "snn_rpn_head_forward_readouts_typed": (C.c_int, [C.POINTER(snn_rpn_level), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                                      C.POINTER(snn_params)] + [C.c_void_p] * 8 + [C.c_size_t, c_stream]),
    "snn_det_head_forward_k_typed": (C.c_int, [C.c_void_p] + [C.c_int] * 7 + [C.POINTER(snn_params), C.c_void_p, C.c_int] +
                                     [C.c_void_p] * 9 + [C.c_size_t, c_stream]),
    "snn_det_head_forward_readouts_typed": (C.c_int, [C.c_void_p] + [C.c_int] * 6 + [C.c_void_p, C.c_int, C.POINTER(snn_params),
                                                      C.c_void_p, C.c_int] + [C.c_void_p] * 9 + [C.c_size_t, c_stream]),
    "snn_det_head_forward_roialign_k_typed": (C.c_int, [C.POINTER(snn_roi_level), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                                        C.c_void_p] + [C.c_int] * 5 + [C.POINTER(snn_params), C.c_void_p, C.c_int] +
                                              [C.c_void_p] * 9 + [C.c_size_t, c_stream]),
    "snn_det_head_forward_roialign_readouts_typed": (C.c_int, [C.POINTER(snn_roi_level), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                                               C.c_void_p] + [C.c_int] * 4 + [C.c_void_p, C.c_int, C.POINTER(snn_params),
                                                               C.c_void_p, C.c_int] + [C.c_void_p] * 9 + [C.c_size_t, c_stream]),
    # the RPN head with its conv route chosen per call (sparse / dense / decided on the device): the typed forward's arguments without the
    # stage mask, then route, crossover, route_stat (device int32[4])
    "snn_rpn_head_workspace_bytes_routed": (C.c_size_t, [C.POINTER(snn_rpn_level), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "snn_rpn_head_forward_routed": (C.c_int, [C.POINTER(snn_rpn_level), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                              C.POINTER(snn_params), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_float,
                                              C.c_void_p, c_stream]),
    # the detector head with its fc6 route chosen per call: the typed forwards' arguments, then route, crossover, route_stat (device int32[4])
    "snn_det_head_workspace_bytes_routed": (C.c_size_t, [C.c_int] * 8),
    "snn_det_head_forward_routed": (C.c_int, [C.c_void_p] + [C.c_int] * 7 + [C.POINTER(snn_params), C.c_void_p, C.c_int] +
                                    [C.c_void_p] * 9 + [C.c_size_t, C.c_int, C.c_float, C.c_void_p, c_stream]),
    "snn_det_head_forward_roialign_routed": (C.c_int, [C.POINTER(snn_roi_level), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                                       C.c_void_p] + [C.c_int] * 5 + [C.POINTER(snn_params), C.c_void_p, C.c_int] +
                                             [C.c_void_p] * 9 + [C.c_size_t, C.c_int, C.c_float, C.c_void_p, c_stream]),
    "snn_encode_nchw_typed": (C.c_int, [C.c_void_p] + [C.c_int] * 6 + [C.POINTER(snn_params), C.c_void_p, C.c_size_t, c_stream]),
    "snn_roi_align_encode_typed": (C.c_int, [C.POINTER(snn_roi_level), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_int, C.c_int, C.POINTER(snn_params), C.c_void_p, C.c_size_t, C.c_void_p, c_stream]),
    # spike taps (taps.py): where a head pass leaves its hidden spike planes (host-only queries), then counts and rasters read through a view
    "snn_rpn_head_planes_view": (C.c_int, [C.POINTER(snn_rpn_level), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(snn_params), C.c_int, C.c_int,
                                           C.POINTER(snn_planes_view)]),
    "snn_det_head_planes_view": (C.c_int, [C.c_int] * 6 + [C.POINTER(snn_params), C.c_int, C.c_int, C.c_int, C.POINTER(snn_planes_view),
                                                           C.POINTER(snn_planes_view)]),
    "snn_planes_counts": (C.c_int, [C.c_void_p, C.POINTER(snn_planes_view), C.POINTER(C.c_int64), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                    C.c_void_p, c_stream]),
    "snn_planes_raster_nchw": (C.c_int, [C.c_void_p, C.POINTER(snn_planes_view), C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                         c_stream]),
    "snn_planes_raster_rows": (C.c_int, [C.c_void_p, C.POINTER(snn_planes_view), C.c_int, C.c_int, C.c_void_p, c_stream]),
    # readout weight gradients (readout.py): planes + view, n_cols, T', params, grad_a, grad_b, NA, NB, gw_a, gw_b, accumulate, scratch, its bytes
    "snn_li_heads_wgrad_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int, C.c_int, C.c_int]),
    "snn_li_heads_wgrad": (C.c_int, [C.c_void_p, C.POINTER(snn_planes_view), C.c_int, C.c_int, C.POINTER(snn_params), C.c_void_p, C.c_void_p,
                                     C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, c_stream]),
    # target matching and head losses (losses.py).  match: boxes, box_start (host), gt_boxes, gt_labels, gt_start (host), N, high, low,
    # allow_low_quality, weights (host), matched_idx, label, reg_target, scratch, its bytes
    "snn_match_targets_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int]),
    "snn_match_targets": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.c_int, C.c_float, C.c_float,
                                    C.c_int, C.POINTER(C.c_float), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, c_stream]),
    # levels, n_levels, A, N, logits, deltas, label, sampled, reg_target, loss, g_logits, g_deltas, scratch, its bytes
    "snn_rpn_loss_grad_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "snn_rpn_loss_grad": (C.c_int, [C.POINTER(snn_rpn_level), C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 9 + [C.c_size_t, c_stream]),
    # logits, box, label, reg_target, R, K, K4, loss, g_logits, g_box, scratch, its bytes
    "snn_det_loss_grad_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "snn_det_loss_grad": (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 3 + [C.c_void_p] * 4 + [C.c_size_t, c_stream]),
    # hidden-layer gradients of fc7 -> lif7 (hidden.py).  planes_to_rows: workspace + view, T', out.  lif_surrogate_bwd: cur, ldc, z_rows, Tc, R, N,
    # params, alpha, gz, gu, d_cur.  spike_linear_wgrad: a_rows, d_cur, ldd, T', rows, K, N, gw, accumulate, scratch, its bytes
    "snn_planes_to_rows": (C.c_int, [C.c_void_p, C.POINTER(snn_planes_view), C.c_int, C.c_void_p, c_stream]),
    "snn_lif_surrogate_bwd": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(snn_params), C.c_float, C.c_void_p,
                                        C.c_void_p, C.c_void_p, c_stream]),
    "snn_spike_linear_wgrad_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int, C.c_int, C.c_int]),
    "snn_spike_linear_wgrad": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                         C.c_size_t, c_stream]),
    # the spike-fed weight gradient on the bf16 matrix cores (fc6_grad.py): the argument lists of the fp32 pair above
    "snn_spike_wgrad_bf16x3_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int, C.c_int, C.c_int]),
    "snn_spike_wgrad_bf16x3_slabs": (C.c_int, [C.c_int64, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64)]),
    "snn_spike_wgrad_bf16x3": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                         C.c_size_t, c_stream]),
}

_LIB = None
_STATIC_PATH = ("snn_roi_assign", "snn_det_postprocess_padded", "snn_pack_padded_detections", "snn_debug_last_enc_mode",
                # (an A/B library from before the spike taps: taps.py then raises AttributeError)
                "snn_rpn_head_planes_view", "snn_det_head_planes_view", "snn_planes_counts", "snn_planes_raster_nchw", "snn_planes_raster_rows",
                # (... from before the readout gradients: readout.py then raises AttributeError)
                "snn_li_heads_wgrad_workspace_bytes", "snn_li_heads_wgrad",
                # (... from before the head losses: losses.py then raises AttributeError)
                "snn_match_targets_workspace_bytes", "snn_match_targets", "snn_rpn_loss_grad_workspace_bytes", "snn_rpn_loss_grad",
                "snn_det_loss_grad_workspace_bytes", "snn_det_loss_grad",
                # (... from before the hidden-layer gradients: hidden.py then raises AttributeError)
                "snn_planes_to_rows", "snn_lif_surrogate_bwd", "snn_spike_linear_wgrad_workspace_bytes", "snn_spike_linear_wgrad",
                # (... from before fc6's gradient: fc6_grad.py then raises AttributeError)
                "snn_spike_wgrad_bf16x3_workspace_bytes", "snn_spike_wgrad_bf16x3_slabs", "snn_spike_wgrad_bf16x3")


class SnnHipError(RuntimeError):
    pass


class InexactWeightSplit(SnnHipError):
    """a weight tensor cannot be carried as three bf16 planes exactly (magnitudes with bits below 2^-133, values next to FLT_MAX,
    NaN / infinity): the bf16x3 kernels must not run on it (ops.check_bf16x3_split; the modules fall back to "f32_strict")"""

    def __init__(self, what: str, inexact: int, nonfinite: int):
        super().__init__("%s: %d weight(s) are not exactly hi + mid + lo in bf16, %d are non-finite" % (what, inexact, nonfinite))
        self.inexact, self.nonfinite = inexact, nonfinite


def lib_path() -> str:
    return _build.LIB_PATH


def load(build_if_missing: bool = True):
    """Load libsnnhip.so (building it in-tree if hipcc is available and it is missing/stale)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = os.environ.get("SNN_HIP_LIB", _build.LIB_PATH)      # override: A/B builds of the kernels
    if path == _build.LIB_PATH and build_if_missing and _build.needs_build() and os.path.exists(_build.HIPCC):
        _build.build()
    if not os.path.exists(path):
        raise SnnHipError("libsnnhip.so not found at %s (run `python -m snn_automotive_object_detection_amd.build`); "
                          "there is no CPU fallback" % path)
    lib = C.CDLL(path)
    for name, (res, args) in list(SYMBOLS.items()) + list(DEBUG_SYMBOLS.items()):
        if path != _build.LIB_PATH and (name.endswith("_typed") or name.endswith("_routed") or name in _STATIC_PATH) and not hasattr(lib, name):
            continue                     # an A/B library from before the typed entry points: fp32 features only (half features: AttributeError);
                                         # from before the static-shape path: the list API only; from before snn_debug_last_enc_mode:
                                         # no report of the encoder form; from before the conv route: the sparse route only
        fn = getattr(lib, name)          # AttributeError if the .so does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    _LIB = lib
    return lib


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = load().snn_last_error()
        raise SnnHipError("%s failed (rc=%d): %s" % (what, rc, msg.decode() if msg else "?"))


def reload_knobs():
    """the SNN_* debug knobs are read from the environment once and frozen; tests that flip them call this afterwards"""
    if _LIB is not None:
        _LIB.snn_debug_reload_knobs()
