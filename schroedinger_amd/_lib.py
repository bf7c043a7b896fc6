"""ctypes binding of libschro_hip.so -- the declarations of include/schro_hip.h.

There is no CPU fallback: if the HIP library is missing or cannot be loaded,
importing the operators raises.  Nothing here touches oracle/.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# SCHRO_HIP_LIB: another build of the same library (A/B runs of kernel variants on the GPU box)
LIB_PATH = os.environ.get("SCHRO_HIP_LIB") or os.path.join(_HERE, "libschro_hip.so")

# every extern "C" symbol include/schro_hip.h declares
EXPORTED_SYMBOLS = [
    "schro_hip_context_new", "schro_hip_context_free", "schro_hip_device_count",
    "schro_hip_last_error", "schro_hip_set_abort_on_error", "schro_hip_init", "schro_hip_thread_bind", "schro_hip_thread_bound", "schro_hip_context_set_stage_completion", "schro_hip_dequant_plan_new", "schro_hip_dequant_plan_run", "schro_hip_dequant_plan_free", "schro_hip_queue_mark_synchronize",
    "schro_hip_host_alloc", "schro_hip_host_free", "schro_hip_upload_2d_async", "schro_hip_download_2d_async",
    "schro_hip_queue_synchronize", "schro_hip_queue_set_cu_mask", "schro_memory_domain_new_hip_host", "schro_hip_codeblock_layout",
    "schro_frame_to_hip_async", "schro_hipframe_to_cpu_async", "schro_hip_frame_copy_to",
    "schro_upsampled_hipframe_upsample_inplace",
    "schro_hip_scheduler_new_on", "schro_hip_scheduler_publish_reference", "schro_hip_scheduler_reference_frame",
    "schro_hip_scheduler_moves", "schro_hip_scheduler_skipped", "schro_hip_scheduler_refs_in_flight_max",
    "schro_hip_domain_alloc", "schro_hip_domain_free", "schro_hip_domain_bytes",
    "schro_hip_upload_2d", "schro_hip_download_2d", "schro_hip_memset",
    "schro_hip_synchronize", "schro_hip_stream",
    "schro_memory_domain_new_hip", "schro_memory_domain_free_hip", "schro_hip_domain_context",
    "schro_hip_context_domain",
    "schro_hip_obmc_stamps_dump",
    "schro_hip_scheduler_new", "schro_hip_scheduler_new_virtual", "schro_hip_scheduler_free",
    "schro_hip_scheduler_n_devices", "schro_hip_scheduler_context", "schro_hip_scheduler_submit",
    "schro_hip_scheduler_retire", "schro_hip_scheduler_wait",
    "schro_hip_context_select_queue", "schro_hip_context_queue", "schro_hip_queue_wait",
    "schro_hip_queue_mark", "schro_hip_queue_wait_mark",
    "schro_hip_timer_begin", "schro_hip_timer_end",
    "schro_hip_profile_enable", "schro_hip_profile_reset", "schro_hip_profile_read", "schro_hip_obmc_routes",
    "schro_hip_v210_routes", "schro_hip_pack8_routes", "schro_hip_wide_routes", "schro_hip_unpack_routes",
    "schro_hip_unpack_batch", "schro_hip_unpack_iwt_batch",
    "schro_hip_iiwt_batch", "schro_hip_iwt_batch", "schro_hipframe_iwt_transform", "schro_hip_convert_u8_batch", "schro_hip_upsample_batch",
    "schro_hip_downsample_batch", "schro_hip_metric_scan_setup", "schro_hip_metric_scan_batch", "schro_hipframe_downsample",
    "schro_rough_me_heirarchical_scan_nohint_hip",
    "schro_hip_rough_hint_batch", "schro_hip_rough_me_batch", "schro_hip_rough_hint_check", "schro_hip_rough_me_check",
    "schro_rough_me_heirarchical_scan_hint_hip", "schro_rough_me_heirarchical_scan_hip",
    "schro_hip_hbm_level_batch", "schro_hip_hbm_batch", "schro_hip_hbm_level_check", "schro_hip_hbm_check",
    "schro_hierarchical_bm_scan_hint_hip", "schro_hbm_scan_hip",
    "schro_hip_subpel_error_batch", "schro_hip_subpel_choose_batch", "schro_hip_subpel_batch", "schro_hip_subpel_check",
    "schro_encoder_motion_predict_subpel_deep_hip",
    "schro_hip_split2_metric_batch", "schro_hip_split2_choose_batch", "schro_hip_split2_batch", "schro_hip_split2_check",
    "schro_mode_decision_split2_hip",
    "schro_hip_mode_metric_batch", "schro_hip_mode_choose_batch", "schro_hip_mode_decision_batch", "schro_hip_mode_decision_check",
    "schro_mode_decision_hip",
    "schro_hip_upsampled_bytes", "schro_hip_upsampled_download", "schro_hip_upsampled_pair_bytes",
    "schro_hip_upsampled_pair_download", "schro_hip_pack_u8_batch",
    "schro_hip_pack_v210_batch", "schro_hip_iiwt_pack_v210_batch", "schro_hip_iiwt_pack_u8_batch", "schro_hip_pack_wide_batch", "schro_hip_shift_right_batch",
    "schro_hip_iiwt_pack_wide_batch",
    "schro_hipframe_shift_right", "schro_hip_add_batch", "schro_hipframe_add",
    "schro_hip_lowdelay_arith", "schro_hip_lowdelay_batch", "schro_hip_dc_predict_batch",
    "schro_hip_lowdelay_encode_batch", "schro_hip_encode_lowdelay_transform_data",
    "schro_hip_noarith_encode_bound", "schro_hip_noarith_encode_batch", "schro_hip_noarith_encode_check",
    "schro_hip_encode_transform_data_noarith",
    "schro_hip_noarith_decode_batch", "schro_hip_noarith_decode_check", "schro_hip_noarith_decode_scratch_words",
    "schro_hipframe_decode_transform_data_noarith",
    "schro_hip_arith_decode_batch", "schro_hip_arith_decode_check", "schro_hip_arith_decode_scratch_words",
    "schro_hipframe_decode_transform_data_arith",
    "schro_hip_motion_encode_bound", "schro_hip_motion_encode_batch", "schro_hip_motion_encode_check",
    "schro_hip_encode_motion_data_noarith",
    "schro_hip_motion_decode_batch", "schro_hip_motion_decode_check", "schro_hip_motion_decode_scratch_words",
    "schro_hip_decode_motion_data_noarith",
    "schro_hip_motion_arith_decode_batch", "schro_hip_motion_arith_decode_check", "schro_hip_motion_arith_decode_scratch_words",
    "schro_hip_decode_motion_data_arith",
    "schro_hip_dequant_batch", "schro_hip_quantise_batch", "schro_hip_subtract_batch", "schro_hipframe_subtract",
    "schro_hipframe_quantise", "schro_hip_histogram_batch", "schro_hipframe_subband_histograms",
    "schro_hip_quant_choose_tables", "schro_hip_quant_choose_batch", "schro_hip_quant_choose_check",
    "schro_hip_quantise_chosen_batch", "schro_hip_noarith_encode_chosen_batch", "schro_hip_noarith_encode_chosen_check",
    "schro_encoder_choose_quantisers_hip",
    "schro_hip_decode_lowdelay_transform_data", "schro_hipframe_dequantise",
    "schro_hip_obmc_batch", "schro_hip_obmc_prediction_epoch", "schro_hip_obmc_overflowed",
    "schro_hip_frame_new_and_alloc", "schro_hip_frame_ref", "schro_hip_frame_unref",
    "schro_frame_to_hip", "schro_hipframe_to_cpu",
    "schro_frame_inverse_iwt_transform_hip", "schro_frame_inverse_iwt_transform_combine_hip", "schro_frame_inverse_iwt_transform_convert_hip",
    "schro_frame_inverse_iwt_transform_combine_convert_hip", "schro_frame_inverse_iwt_transform_shift_convert_hip",
    "schro_upsampled_hipframe_upsample",
    "schro_motion_render_hip", "schro_hipframe_convert", "schro_hipframe_convert_input", "schro_hipframe_unpack_iwt_transform",
    "schro_hip_unpack_geometry",
    "schro_hip_plane_sums_batch", "schro_hip_plane_sums_check", "schro_hip_lowpass2_coeff", "schro_hip_lowpass2_batch",
    "schro_hip_lowpass2_check", "schro_hip_ssim_scratch_bytes", "schro_hip_picture_stats_geometry", "schro_hip_ssim_batch", "schro_hip_ssim_check",
    "schro_hipframe_calculate_average_luma", "schro_hipframe_mean_squared_error", "schro_hipframe_ssim",
    "schro_hipframe_filter_lowpass2", "schro_engine_get_scene_change_score_hip",
]


class IwtPlane(C.Structure):
    _fields_ = [("src", C.c_void_p), ("src_stride", C.c_int),
                ("dst", C.c_void_p), ("dst_stride", C.c_int),
                ("width", C.c_int), ("height", C.c_int),
                ("pred", C.c_void_p), ("pred_stride", C.c_int),
                ("out_width", C.c_int), ("out_height", C.c_int), ("combine", C.c_int),
                ("ll", C.c_void_p), ("ll_stride", C.c_int), ("reserved", C.c_int)]


class IwtFwdPlane(C.Structure):
    _fields_ = [("src", C.c_void_p), ("src_stride", C.c_int),
                ("dst", C.c_void_p), ("dst_stride", C.c_int),
                ("width", C.c_int), ("height", C.c_int)]


class DownsamplePlane(C.Structure):
    _fields_ = [("src", C.c_void_p), ("src_stride", C.c_int), ("src_width", C.c_int), ("src_height", C.c_int),
                ("dst", C.c_void_p), ("dst_stride", C.c_int), ("dst_extension", C.c_int)]


class SumsJob(C.Structure):
    """SchroHipSumsJob: one plane (and its optional second plane) of schro_hip_plane_sums_batch."""
    _fields_ = [("a", C.c_void_p), ("a_stride", C.c_int), ("bytes_per_sample", C.c_int), ("width", C.c_int), ("height", C.c_int),
                ("b", C.c_void_p), ("b_stride", C.c_int), ("b_width", C.c_int), ("b_height", C.c_int), ("result", C.c_void_p)]


class Lowpass2Plane(C.Structure):
    """SchroHipLowpass2Plane: one plane of schro_hip_lowpass2_batch."""
    _fields_ = [("data", C.c_void_p), ("stride", C.c_int), ("bytes_per_sample", C.c_int), ("width", C.c_int), ("height", C.c_int),
                ("h_coeff", C.c_double * 4), ("v_coeff", C.c_double * 4), ("out_of_range", C.c_void_p)]


class SsimResult(C.Structure):
    _fields_ = [("sum", C.c_double), ("out_of_range", C.c_uint32 * 5), ("reserved", C.c_uint32)]


class SsimPicture(C.Structure):
    """SchroHipSsimPicture: one picture of schro_hip_ssim_batch."""
    _fields_ = [("a", C.c_void_p), ("a_stride", C.c_int), ("width", C.c_int), ("height", C.c_int),
                ("b", C.c_void_p), ("b_stride", C.c_int), ("b_width", C.c_int), ("b_height", C.c_int),
                ("scratch", C.c_void_p), ("scratch_bytes", C.c_size_t), ("result", C.c_void_p),
                ("map", C.c_void_p), ("map_stride", C.c_int)]


class MetricScan(C.Structure):
    """The input members of SchroMetricScan (schrometric.h:38-53)."""
    _fields_ = [(n, C.c_int) for n in ("x", "y", "block_width", "block_height", "ref_x", "ref_y", "scan_width", "scan_height",
                                       "gravity_x", "gravity_y", "dx", "dy")]


class MetricScanResult(C.Structure):
    _fields_ = [("dx", C.c_int), ("dy", C.c_int), ("metric", C.c_uint32), ("reserved", C.c_uint32)]


class MetricScanPicture(C.Structure):
    _fields_ = [("frame", C.c_void_p), ("frame_stride", C.c_int), ("ref", C.c_void_p), ("ref_stride", C.c_int),
                ("width", C.c_int), ("height", C.c_int), ("extension", C.c_int),
                ("scans", C.POINTER(MetricScan)), ("nscans", C.c_int),
                ("results", C.c_void_p), ("metrics", C.c_void_p)]


MAX_HIER_LEVELS = 8             # SCHRO_HIP_MAX_HIER_LEVELS


class RoughPlane(C.Structure):
    """The luma planes of a frame and its reference at one pyramid level."""
    _fields_ = [("frame", C.c_void_p), ("frame_stride", C.c_int), ("ref", C.c_void_p), ("ref_stride", C.c_int),
                ("width", C.c_int), ("height", C.c_int), ("extension", C.c_int)]


class RoughHintPicture(C.Structure):
    _fields_ = [("frame", C.c_void_p), ("frame_stride", C.c_int), ("ref", C.c_void_p), ("ref_stride", C.c_int),
                ("width", C.c_int), ("height", C.c_int), ("extension", C.c_int),
                ("x_num_blocks", C.c_int), ("y_num_blocks", C.c_int), ("xbsep_luma", C.c_int), ("ybsep_luma", C.c_int),
                ("shift", C.c_int), ("distance", C.c_int), ("ref_index", C.c_int),
                ("hint_field", C.c_void_p), ("field", C.c_void_p)]


class RoughChain(C.Structure):
    _fields_ = [("n_levels", C.c_int), ("levels", C.POINTER(RoughPlane)),
                ("x_num_blocks", C.c_int), ("y_num_blocks", C.c_int), ("xbsep_luma", C.c_int), ("ybsep_luma", C.c_int),
                ("ref_index", C.c_int), ("fields", C.c_void_p * MAX_HIER_LEVELS)]


class HbmPlane(C.Structure):
    """The three components of a frame and its reference at one pyramid level."""
    _fields_ = [("frame", C.c_void_p * 3), ("frame_stride", C.c_int * 3), ("ref", C.c_void_p * 3), ("ref_stride", C.c_int * 3),
                ("width", C.c_int), ("height", C.c_int), ("h_shift", C.c_int), ("v_shift", C.c_int), ("extension", C.c_int)]


class HbmLevel(C.Structure):
    _fields_ = [("plane", HbmPlane),
                ("x_num_blocks", C.c_int), ("y_num_blocks", C.c_int), ("xbsep_luma", C.c_int), ("ybsep_luma", C.c_int),
                ("shift", C.c_int), ("h_range", C.c_int), ("ref_index", C.c_int),
                ("hint_field", C.c_void_p), ("field", C.c_void_p)]


class HbmChain(C.Structure):
    _fields_ = [("n_levels", C.c_int), ("levels", C.POINTER(HbmPlane)),
                ("x_num_blocks", C.c_int), ("y_num_blocks", C.c_int), ("xbsep_luma", C.c_int), ("ybsep_luma", C.c_int),
                ("ref_index", C.c_int), ("fields", C.c_void_p * (MAX_HIER_LEVELS + 1))]


class SubpelChain(C.Structure):
    """One (picture, reference) pair of the sub-pel refinement."""
    _fields_ = [("src", C.c_void_p), ("src_stride", C.c_int), ("ref_up", C.c_void_p), ("ref_up_stride", C.c_int),
                ("width", C.c_int), ("height", C.c_int), ("extension", C.c_int),
                ("x_num_blocks", C.c_int), ("y_num_blocks", C.c_int), ("xbsep_luma", C.c_int), ("ybsep_luma", C.c_int),
                ("mv_precision", C.c_int), ("ref_index", C.c_int), ("lambda", C.c_double),
                ("src_field", C.c_void_p), ("field", C.c_void_p)]


class Split2Picture(C.Structure):
    """One picture of the split-2 mode decision."""
    _fields_ = [("src", C.c_void_p * 3), ("src_stride", C.c_int * 3), ("num_refs", C.c_int),
                ("ref_up", (C.c_void_p * 3) * 2), ("ref_up_stride", C.c_int * 3),
                ("width", C.c_int), ("height", C.c_int), ("h_shift", C.c_int), ("v_shift", C.c_int), ("extension", C.c_int),
                ("x_num_blocks", C.c_int), ("y_num_blocks", C.c_int), ("xbsep_luma", C.c_int), ("ybsep_luma", C.c_int),
                ("mv_precision", C.c_int), ("chroma_pairs", C.c_int), ("lambda", C.c_double),
                ("fields", C.c_void_p * 2), ("motion", C.c_void_p), ("superblocks", C.c_void_p)]


class ModePicture(C.Structure):
    """One picture of the whole mode decision."""
    _fields_ = [("split2", Split2Picture), ("hbm_fields", (C.c_void_p * 2) * 2), ("trials", C.c_void_p), ("stats", C.c_void_p)]


class ConvertPlane(C.Structure):
    _fields_ = [("src", C.c_void_p), ("src_stride", C.c_int),
                ("dst", C.c_void_p), ("dst_stride", C.c_int),
                ("width", C.c_int), ("height", C.c_int)]


class PackPlane(C.Structure):
    _fields_ = [("src", C.c_void_p * 3), ("src_stride", C.c_int * 3),
                ("src_width", C.c_int), ("src_height", C.c_int),
                ("src_h_shift", C.c_int), ("src_v_shift", C.c_int),
                ("dst", C.c_void_p), ("dst_stride", C.c_int),
                ("width", C.c_int), ("height", C.c_int), ("format", C.c_int)]


class UnpackPicture(C.Structure):
    """SchroHipUnpackPicture (include/schro_hip.h): one picture of schro_hip_unpack_batch."""
    _fields_ = [("src", C.c_void_p * 3), ("src_stride", C.c_int * 3), ("format", C.c_int),
                ("src_width", C.c_int), ("src_height", C.c_int), ("src_bpp", C.c_int),
                ("src_h_shift", C.c_int), ("src_v_shift", C.c_int), ("reserved", C.c_int),
                ("dst", C.c_void_p * 3), ("dst_stride", C.c_int * 3), ("dst_bpp", C.c_int),
                ("h_shift", C.c_int), ("v_shift", C.c_int), ("width", C.c_int), ("height", C.c_int)]


class UnpackIwtPicture(C.Structure):
    """SchroHipUnpackIwtPicture (include/schro_hip.h): one picture of schro_hip_unpack_iwt_batch."""
    _fields_ = [("src", C.c_void_p), ("src_stride", C.c_int), ("format", C.c_int),
                ("src_width", C.c_int), ("src_height", C.c_int), ("width", C.c_int), ("height", C.c_int),
                ("dst", C.c_void_p * 3), ("dst_stride", C.c_int * 3), ("iwt_width", C.c_int), ("iwt_height", C.c_int),
                ("h_shift", C.c_int), ("v_shift", C.c_int), ("reserved", C.c_int)]


class IwtPackPicture(C.Structure):
    _fields_ = [("src", C.c_void_p * 3), ("src_stride", C.c_int * 3), ("width", C.c_int), ("height", C.c_int),
                ("h_shift", C.c_int), ("v_shift", C.c_int), ("dst", C.c_void_p), ("dst_stride", C.c_int),
                ("out_width", C.c_int), ("out_height", C.c_int)]


class IwtPack8Picture(C.Structure):
    _fields_ = [("src", C.c_void_p * 3), ("src_stride", C.c_int * 3), ("width", C.c_int), ("height", C.c_int),
                ("h_shift", C.c_int), ("v_shift", C.c_int), ("pred", C.c_void_p * 3), ("pred_stride", C.c_int * 3),
                ("dst", C.c_void_p), ("dst_stride", C.c_int), ("out_width", C.c_int), ("out_height", C.c_int),
                ("format", C.c_int)]


class IwtPackWidePicture(C.Structure):
    _fields_ = [("src", C.c_void_p * 3), ("src_stride", C.c_int * 3), ("width", C.c_int), ("height", C.c_int),
                ("h_shift", C.c_int), ("v_shift", C.c_int), ("dst", C.c_void_p), ("dst_stride", C.c_int),
                ("out_width", C.c_int), ("out_height", C.c_int), ("format", C.c_int), ("shift", C.c_int)]


class LowDelayParams(C.Structure):
    _fields_ = [("transform_depth", C.c_int),
                ("iwt_luma_width", C.c_int), ("iwt_luma_height", C.c_int),
                ("iwt_chroma_width", C.c_int), ("iwt_chroma_height", C.c_int),
                ("n_horiz_slices", C.c_int), ("n_vert_slices", C.c_int),
                ("slice_bytes_num", C.c_int), ("slice_bytes_denom", C.c_int),
                ("quant_matrix", C.c_int * 19)]


class LowDelayPicture(C.Structure):
    _fields_ = [("slices", C.c_void_p), ("slices_bytes", C.c_size_t),
                ("comp", C.c_void_p * 3), ("stride", C.c_int * 3)]


class LowDelayEncodePicture(C.Structure):
    _fields_ = [("comp", C.c_void_p * 3), ("stride", C.c_int * 3),
                ("slices", C.c_void_p), ("slices_bytes", C.c_size_t),
                ("base_index", C.c_void_p), ("overruns", C.c_void_p)]


class Codeblock(C.Structure):
    _fields_ = [("dst_offset", C.c_int), ("dst_stride", C.c_int), ("width", C.c_int), ("height", C.c_int),
                ("src_offset", C.c_int), ("src_bytes", C.c_ubyte), ("quant_index", C.c_ubyte),
                ("pad", C.c_ubyte * 2)]


class DequantPlane(C.Structure):
    _fields_ = [("dst", C.c_void_p), ("values", C.c_void_p), ("codeblocks", C.POINTER(Codeblock)),
                ("ncodeblocks", C.c_int), ("is_intra", C.c_int)]


class CodeblockSummary(C.Structure):
    _fields_ = [("nonzero", C.c_uint32), ("max_abs", C.c_uint32)]


class QuantPlane(C.Structure):
    """SchroHipQuantPlane (include/schro_hip.h): one component of schro_hip_quantise_batch."""
    _fields_ = [("coeffs", C.c_void_p), ("quant", C.c_void_p), ("bytes", C.c_size_t), ("codeblocks", C.POINTER(Codeblock)),
                ("ncodeblocks", C.c_int), ("is_intra", C.c_int), ("dc_predict_first", C.c_int), ("dc_width", C.c_int),
                ("dc_height", C.c_int), ("summary", C.c_void_p)]


NOARITH_MAX_SUBBANDS = 19       # SCHRO_HIP_NOARITH_MAX_SUBBANDS (include/schro_hip.h)


class NoarithResult(C.Structure):
    """SchroHipNoarithResult: what schro_hip_noarith_encode_batch leaves on the device per picture."""
    _fields_ = [("bytes", C.c_uint32), ("overrun", C.c_uint32), ("false_zero_codeblocks", C.c_uint32),
                ("false_zero_subbands", C.c_uint32), ("subband_bits", (C.c_uint32 * NOARITH_MAX_SUBBANDS) * 3)]


class NoarithPicture(C.Structure):
    """SchroHipNoarithPicture (include/schro_hip.h): one picture of schro_hip_noarith_encode_batch."""
    _fields_ = [("quant", C.c_void_p * 3), ("bytes", C.c_size_t * 3), ("stride", C.c_int * 3), ("iwt_width", C.c_int * 3),
                ("iwt_height", C.c_int * 3), ("codeblocks", C.POINTER(Codeblock) * 3), ("ncodeblocks", C.c_int * 3),
                ("transform_depth", C.c_int), ("horiz_codeblocks", C.c_int * 7), ("vert_codeblocks", C.c_int * 7),
                ("codeblock_mode_index", C.c_int), ("out", C.c_void_p), ("capacity", C.c_size_t), ("result", C.c_void_p)]


class NoarithDecodeResult(C.Structure):
    """SchroHipNoarithDecodeResult: what schro_hip_noarith_decode_batch leaves on the device per picture."""
    _fields_ = [("bytes_read", C.c_uint32), ("error", C.c_uint32), ("first_error", C.c_uint32), ("compat_quant_offset", C.c_uint32),
                ("truncated", C.c_uint32), ("not_consumed", C.c_uint32), ("overran", C.c_uint32), ("long_codes", C.c_uint32),
                ("clamped_quant", C.c_uint32), ("subband_length", (C.c_uint32 * NOARITH_MAX_SUBBANDS) * 3),
                ("subband_quant_index", (C.c_uint8 * NOARITH_MAX_SUBBANDS) * 3)]


class NoarithDecodePicture(C.Structure):
    """SchroHipNoarithDecodePicture (include/schro_hip.h): one picture of schro_hip_noarith_decode_batch."""
    _fields_ = [("data", C.c_void_p), ("data_bytes", C.c_size_t), ("bytes_on_device", C.c_void_p), ("coeffs", C.c_void_p * 3),
                ("bytes", C.c_size_t * 3), ("stride", C.c_int * 3), ("quant", C.c_void_p * 3), ("iwt_width", C.c_int * 3),
                ("iwt_height", C.c_int * 3), ("transform_depth", C.c_int), ("horiz_codeblocks", C.c_int * 7),
                ("vert_codeblocks", C.c_int * 7), ("codeblock_mode_index", C.c_int), ("is_intra", C.c_int),
                ("compat_quant_offset", C.c_int), ("result", C.c_void_p)]


class ArithDecodeResult(C.Structure):
    """SchroHipArithDecodeResult: what schro_hip_arith_decode_batch leaves on the device per picture."""
    _fields_ = NoarithDecodeResult._fields_ + [("bins", C.c_uint32)]


class ArithDecodePicture(C.Structure):
    """SchroHipArithDecodePicture (include/schro_hip.h): one picture of schro_hip_arith_decode_batch."""
    _fields_ = NoarithDecodePicture._fields_


MOTION_SECTIONS = 9             # SCHRO_HIP_MOTION_SECTIONS (include/schro_hip.h)


class MotionEncodeResult(C.Structure):
    """SchroHipMotionEncodeResult: what schro_hip_motion_encode_batch leaves on the device per picture."""
    _fields_ = [("bytes", C.c_uint32), ("overrun", C.c_uint32), ("section_bytes", C.c_uint32 * MOTION_SECTIONS),
                ("section_units", C.c_uint32 * MOTION_SECTIONS), ("asserted", C.c_uint32), ("unverified", C.c_uint32),
                ("first_unverified", C.c_int32)]


class MotionEncodePicture(C.Structure):
    """SchroHipMotionEncodePicture (include/schro_hip.h): one picture of schro_hip_motion_encode_batch."""
    _fields_ = [("motion", C.c_void_p), ("x_num_blocks", C.c_int), ("y_num_blocks", C.c_int), ("num_refs", C.c_int),
                ("have_global_motion", C.c_int), ("out", C.c_void_p), ("capacity", C.c_size_t), ("result", C.c_void_p)]


class MotionDecodeResult(C.Structure):
    """SchroHipMotionDecodeResult: what schro_hip_motion_decode_batch leaves on the device per picture."""
    _fields_ = [("bytes", C.c_uint32), ("section_bytes", C.c_uint32 * MOTION_SECTIONS),
                ("section_units", C.c_uint32 * MOTION_SECTIONS), ("section_bits", C.c_uint32 * MOTION_SECTIONS),
                ("truncated", C.c_uint32), ("overran", C.c_uint32), ("not_consumed", C.c_uint32), ("long_codes", C.c_uint32),
                ("unverified", C.c_uint32), ("first_unverified", C.c_int32)]


class MotionDecodePicture(C.Structure):
    """SchroHipMotionDecodePicture (include/schro_hip.h): one picture of schro_hip_motion_decode_batch."""
    _fields_ = [("data", C.c_void_p), ("data_bytes", C.c_size_t), ("bytes_on_device", C.c_void_p), ("x_num_blocks", C.c_int),
                ("y_num_blocks", C.c_int), ("num_refs", C.c_int), ("have_global_motion", C.c_int), ("motion", C.c_void_p),
                ("result", C.c_void_p)]


class MotionArithDecodeResult(C.Structure):
    """SchroHipMotionArithDecodeResult: what schro_hip_motion_arith_decode_batch leaves on the device per picture."""
    _fields_ = [("bytes", C.c_uint32), ("section_bytes", C.c_uint32 * MOTION_SECTIONS),
                ("section_units", C.c_uint32 * MOTION_SECTIONS), ("section_offset", C.c_uint32 * MOTION_SECTIONS),
                ("section_bins", C.c_uint32 * MOTION_SECTIONS), ("truncated", C.c_uint32), ("overran", C.c_uint32),
                ("not_consumed", C.c_uint32), ("long_codes", C.c_uint32), ("unverified", C.c_uint32), ("first_unverified", C.c_int32)]


class MotionArithDecodePicture(C.Structure):
    """SchroHipMotionArithDecodePicture (include/schro_hip.h): one picture of schro_hip_motion_arith_decode_batch."""
    _fields_ = MotionDecodePicture._fields_


HISTOGRAM_BINS = 104           # SCHRO_HIP_HISTOGRAM_BINS (include/schro_hip.h)


class HistogramCounts(C.Structure):
    """SchroHipHistogramCounts: raw counts of one sub-band, before the scale by skip."""
    _fields_ = [("bins", C.c_uint32 * HISTOGRAM_BINS), ("overflow", C.c_uint32)]


class HistogramBand(C.Structure):
    _fields_ = [("offset", C.c_int), ("stride", C.c_int), ("width", C.c_int), ("height", C.c_int), ("skip", C.c_int),
                ("dc_predict", C.c_int)]


class HistogramPlane(C.Structure):
    """SchroHipHistogramPlane (include/schro_hip.h): one component of schro_hip_histogram_batch."""
    _fields_ = [("coeffs", C.c_void_p), ("bytes", C.c_size_t), ("bands", C.POINTER(HistogramBand)), ("nbands", C.c_int),
                ("counts", C.c_void_p)]


class Histogram(C.Structure):
    """SchroHipHistogram: layout-identical to the reference's SchroHistogram."""
    _fields_ = [("n", C.c_int), ("bins", C.c_double * HISTOGRAM_BINS)]


QUANT_CHOOSE_INDICES = 60      # SCHRO_HIP_QUANT_CHOOSE_INDICES
QUANT_CHOOSE_BANDS = 19        # SCHRO_HIP_NOARITH_MAX_SUBBANDS
QUANT_ENGINE_LAMBDA, QUANT_ENGINE_BIT_ALLOCATION, QUANT_ENGINE_CONSTANT_ERROR = 0, 1, 2


class QuantChoice(C.Structure):
    """SchroHipQuantChoice (include/schro_hip.h): what schro_hip_quant_choose_batch leaves per picture, on the device."""
    _fields_ = [("frame_lambda", C.c_double), ("sum", C.c_double),
                ("chosen_entropy", C.c_double * QUANT_CHOOSE_BANDS * 3), ("chosen_error", C.c_double * QUANT_CHOOSE_BANDS * 3),
                ("quant_index", C.c_int32 * QUANT_CHOOSE_BANDS * 3), ("evaluations", C.c_int32), ("not_bracketed", C.c_int32),
                ("reserved", C.c_int32)]


class QuantChoosePicture(C.Structure):
    """SchroHipQuantChoosePicture (include/schro_hip.h): one picture of schro_hip_quant_choose_batch."""
    _fields_ = [("counts", C.c_void_p * 3), ("skip", C.c_int * QUANT_CHOOSE_BANDS), ("transform_depth", C.c_int),
                ("is_intra", C.c_int), ("is_noarith", C.c_int), ("engine", C.c_int),
                ("subband_weight", C.c_double * QUANT_CHOOSE_BANDS), ("context_ratio", C.c_double * QUANT_CHOOSE_BANDS * 3),
                ("subband0_lambda_scale", C.c_double), ("chroma_lambda_scale", C.c_double), ("diagonal_lambda_scale", C.c_double),
                ("target", C.c_double), ("result", C.c_void_p), ("est_entropy", C.c_void_p), ("est_error", C.c_void_p)]


class QuantChooseSettings(C.Structure):
    """SchroHipQuantChooseSettings (include/schro_hip.h): what schro_encoder_choose_quantisers_hip takes beside frame and params."""
    _fields_ = [("is_noarith", C.c_int), ("engine", C.c_int), ("target", C.c_double),
                ("subband_weight", C.c_double * QUANT_CHOOSE_BANDS), ("context_ratio", C.c_double * QUANT_CHOOSE_BANDS * 3),
                ("subband0_lambda_scale", C.c_double), ("chroma_lambda_scale", C.c_double), ("diagonal_lambda_scale", C.c_double)]


class QuantisedPicture(C.Structure):
    """SchroHipQuantisedPicture (include/schro_hip.h): a picture's codeblock records and quantised values per component."""
    _fields_ = [("codeblocks", C.POINTER(Codeblock) * 3), ("ncodeblocks", C.c_int * 3), ("values", C.c_void_p * 3),
                ("values_bytes", C.c_size_t * 3), ("values_on_device", C.c_int)]


class DcPlane(C.Structure):
    _fields_ = [("data", C.c_void_p), ("stride", C.c_int), ("width", C.c_int), ("height", C.c_int)]


class UpsamplePlane(C.Structure):
    _fields_ = [("src", C.c_void_p), ("src_stride", C.c_int),
                ("dst", C.c_void_p), ("dst_stride", C.c_int),
                ("width", C.c_int), ("height", C.c_int),
                ("src_v", C.c_void_p), ("src_v_stride", C.c_int)]


class ObmcPlane(C.Structure):
    _fields_ = [("mvs", C.c_void_p),
                ("x_num_blocks", C.c_int), ("y_num_blocks", C.c_int),
                ("xblen_luma", C.c_int), ("yblen_luma", C.c_int),
                ("xbsep_luma", C.c_int), ("ybsep_luma", C.c_int),
                ("mv_precision", C.c_int),
                ("picture_weight_bits", C.c_int), ("picture_weight_1", C.c_int),
                ("picture_weight_2", C.c_int),
                ("chroma_h_shift", C.c_int), ("chroma_v_shift", C.c_int),
                ("component", C.c_int),
                ("ref1", C.c_void_p), ("ref1_stride", C.c_int),
                ("ref2", C.c_void_p), ("ref2_stride", C.c_int),
                ("residual", C.c_void_p), ("residual_stride", C.c_int),
                ("residual_bpp", C.c_int),
                ("out", C.c_void_p), ("out_stride", C.c_int),
                ("width", C.c_int), ("height", C.c_int), ("ref_pair", C.c_int), ("prediction_only", C.c_int)]


class FrameData(C.Structure):
    _fields_ = [("format", C.c_int), ("data", C.c_void_p), ("stride", C.c_int),
                ("width", C.c_int), ("height", C.c_int), ("length", C.c_int),
                ("h_shift", C.c_int), ("v_shift", C.c_int)]


class MemoryDomain(C.Structure):
    """The head of SchroHipMemoryDomain == SchroMemoryDomain (schrodomain.h:13-28): the alloc / free table."""
    _fields_ = [("mutex", C.c_void_p), ("flags", C.c_uint),
                ("alloc", C.CFUNCTYPE(C.c_void_p, C.c_int)),
                ("alloc_2d", C.CFUNCTYPE(C.c_void_p, C.c_int, C.c_int, C.c_int)),
                ("free", C.CFUNCTYPE(None, C.c_void_p, C.c_int))]


class Frame(C.Structure):
    """SchroHipFrame == SchroFrame (schroframe.h:69-94), member for member."""


Frame._fields_ = [("refcount", C.c_int), ("free", C.c_void_p), ("domain", C.c_void_p),
                  ("regions", C.c_void_p * 3), ("priv", C.c_void_p),
                  ("format", C.c_int), ("width", C.c_int), ("height", C.c_int),
                  ("components", FrameData * 3),
                  ("is_virtual", C.c_int), ("cached_lines", (C.c_int * 32) * 3),
                  ("virt_frame1", C.POINTER(Frame)), ("virt_frame2", C.POINTER(Frame)),
                  ("render_line", C.c_void_p), ("virt_priv", C.c_void_p), ("virt_priv2", C.c_void_p),
                  ("extension", C.c_int), ("cache_offset", C.c_int * 3),
                  ("is_upsampled", C.c_int), ("upsample_done", C.c_int)]


class GlobalMotion(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("b0", "b1", "a_exp", "a00", "a01", "a10", "a11", "c_exp", "c0", "c1")]


class Params(C.Structure):
    """SchroHipParams == SchroParams (schroparams.h:31-74)."""
    _fields_ = ([("video_format", C.c_void_p), ("is_noarith", C.c_int), ("wavelet_filter_index", C.c_int),
                 ("transform_depth", C.c_int), ("horiz_codeblocks", C.c_int * 7), ("vert_codeblocks", C.c_int * 7)]
                + [(n, C.c_int) for n in ("codeblock_mode_index", "num_refs", "have_global_motion", "xblen_luma",
                                          "yblen_luma", "xbsep_luma", "ybsep_luma", "mv_precision")]
                + [("global_motion", GlobalMotion * 2)]
                + [(n, C.c_int) for n in ("picture_pred_mode", "picture_weight_bits", "picture_weight_1",
                                          "picture_weight_2", "is_lowdelay", "n_horiz_slices", "n_vert_slices",
                                          "slice_bytes_num", "slice_bytes_denom")]
                + [("quant_matrix", C.c_int * 19)]
                + [(n, C.c_int) for n in ("iwt_chroma_width", "iwt_chroma_height", "iwt_luma_width",
                                          "iwt_luma_height", "x_num_blocks", "y_num_blocks", "x_offset", "y_offset")])


class Motion(C.Structure):
    """SchroHipMotion == SchroMotion (schromotion.h:53-86)."""
    _fields_ = ([("src1", C.POINTER(Frame)), ("src2", C.POINTER(Frame)),
                 ("motion_vectors", C.c_void_p), ("params", C.POINTER(Params))]
                + [(n, C.c_int) for n in ("ref_weight_precision", "ref1_weight", "ref2_weight", "mv_precision",
                                          "xoffset", "yoffset", "xbsep", "ybsep", "xblen", "yblen")]
                + [("block", FrameData), ("alloc_block", FrameData), ("obmc_weight", FrameData),
                   ("alloc_block_ref", FrameData * 2), ("block_ref", FrameData * 2),
                   ("weight_x", C.c_int * 64), ("weight_y", C.c_int * 64)]
                + [(n, C.c_int) for n in ("width", "height", "max_fast_x", "max_fast_y", "simple_weight",
                                          "oneref_noscale")])


# int (*SchroHipPictureFunc) (SchroHipContext *ctx, int device_index, void *priv)
PICTURE_FUNC = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_void_p)

_lib = None


def load():
    """Load libschro_hip.so; raises (never falls back) when it is unavailable."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "schroedinger_amd: %s is missing -- build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` or "
            "`make -C schroedinger_amd/csrc`; there is no CPU fallback" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp, i, sz = C.c_void_p, C.c_int, C.c_size_t
    L.schro_hip_context_new.argtypes = [i]
    L.schro_hip_context_new.restype = vp
    L.schro_hip_context_free.argtypes = [vp]
    L.schro_hip_context_free.restype = None
    L.schro_hip_device_count.restype = i
    L.schro_hip_last_error.restype = C.c_char_p
    L.schro_hip_set_abort_on_error.argtypes = [i]
    L.schro_hip_domain_alloc.argtypes = [vp, sz]
    L.schro_hip_domain_alloc.restype = vp
    L.schro_hip_domain_free.argtypes = [vp, vp]
    L.schro_hip_domain_free.restype = i
    L.schro_hip_domain_bytes.argtypes = [vp]
    L.schro_hip_domain_bytes.restype = sz
    L.schro_hip_upload_2d.argtypes = [vp, vp, i, vp, i, i, i]
    L.schro_hip_upload_2d.restype = i
    L.schro_hip_download_2d.argtypes = [vp, vp, i, vp, i, i, i]
    L.schro_hip_download_2d.restype = i
    L.schro_hip_memset.argtypes = [vp, vp, i, sz]
    L.schro_hip_memset.restype = i
    L.schro_hip_synchronize.argtypes = [vp]
    L.schro_hip_synchronize.restype = i
    L.schro_hip_stream.argtypes = [vp]
    L.schro_hip_stream.restype = vp
    L.schro_memory_domain_new_hip.argtypes = [i]
    L.schro_memory_domain_new_hip.restype = vp
    L.schro_memory_domain_free_hip.argtypes = [vp]
    L.schro_memory_domain_free_hip.restype = None
    L.schro_hip_domain_context.argtypes = [vp]
    L.schro_hip_domain_context.restype = vp
    L.schro_hip_context_domain.argtypes = [vp]
    L.schro_hip_context_domain.restype = vp
    L.schro_hip_init.argtypes = []
    L.schro_hip_init.restype = None
    L.schro_hip_thread_bind.argtypes = [vp]
    L.schro_hip_thread_bind.restype = None
    L.schro_hip_thread_bound.argtypes = []
    L.schro_hip_thread_bound.restype = vp
    L.schro_hip_dequant_plan_new.argtypes = [vp, vp, i, i, i]
    L.schro_hip_dequant_plan_new.restype = vp
    L.schro_hip_dequant_plan_run.argtypes = [vp, vp, i]
    L.schro_hip_dequant_plan_run.restype = i
    L.schro_hip_dequant_plan_free.argtypes = [vp]
    L.schro_hip_dequant_plan_free.restype = None
    L.schro_hip_queue_mark_synchronize.argtypes = [vp, i]
    L.schro_hip_queue_mark_synchronize.restype = i
    L.schro_hip_context_set_stage_completion.argtypes = [vp, i]
    L.schro_hip_context_set_stage_completion.restype = i
    L.schro_hip_host_alloc.argtypes = [C.c_size_t]
    L.schro_hip_host_alloc.restype = vp
    L.schro_hip_host_free.argtypes = [vp]
    L.schro_hip_host_free.restype = None
    L.schro_hip_upload_2d_async.argtypes = [vp, vp, i, vp, i, i, i]
    L.schro_hip_upload_2d_async.restype = i
    L.schro_hip_download_2d_async.argtypes = [vp, vp, i, vp, i, i, i]
    L.schro_hip_download_2d_async.restype = i
    L.schro_hip_queue_synchronize.argtypes = [vp, i]
    L.schro_hip_queue_synchronize.restype = i
    L.schro_hip_queue_set_cu_mask.argtypes = [vp, i, C.POINTER(C.c_uint32), i]
    L.schro_hip_queue_set_cu_mask.restype = i
    L.schro_memory_domain_new_hip_host.argtypes = []
    L.schro_memory_domain_new_hip_host.restype = vp
    L.schro_hip_codeblock_layout.argtypes = [i, i, i, C.POINTER(C.c_int), C.POINTER(C.c_int), i, i, C.POINTER(Codeblock), i]
    L.schro_hip_codeblock_layout.restype = i
    L.schro_frame_to_hip_async.argtypes = [vp, vp]
    L.schro_frame_to_hip_async.restype = i
    L.schro_hipframe_to_cpu_async.argtypes = [vp, vp]
    L.schro_hipframe_to_cpu_async.restype = i
    L.schro_hip_frame_copy_to.argtypes = [vp, vp]
    L.schro_hip_frame_copy_to.restype = vp
    L.schro_upsampled_hipframe_upsample_inplace.argtypes = [vp]
    L.schro_upsampled_hipframe_upsample_inplace.restype = i
    L.schro_hip_scheduler_new_on.argtypes = [C.POINTER(C.c_int), i]
    L.schro_hip_scheduler_new_on.restype = vp
    L.schro_hip_scheduler_publish_reference.argtypes = [vp, i, vp]
    L.schro_hip_scheduler_publish_reference.restype = i
    L.schro_hip_scheduler_reference_frame.argtypes = [vp, i, i]
    L.schro_hip_scheduler_reference_frame.restype = vp
    L.schro_hip_scheduler_moves.argtypes = [vp]
    L.schro_hip_scheduler_moves.restype = C.c_long
    L.schro_hip_scheduler_skipped.argtypes = [vp]
    L.schro_hip_scheduler_skipped.restype = C.c_long
    L.schro_hip_scheduler_refs_in_flight_max.argtypes = [vp]
    L.schro_hip_scheduler_refs_in_flight_max.restype = i
    L.schro_hip_scheduler_new.argtypes = [i]
    L.schro_hip_scheduler_new.restype = vp
    L.schro_hip_scheduler_new_virtual.argtypes = [i]
    L.schro_hip_scheduler_new_virtual.restype = vp
    L.schro_hip_scheduler_free.argtypes = [vp]
    L.schro_hip_scheduler_free.restype = None
    L.schro_hip_scheduler_n_devices.argtypes = [vp]
    L.schro_hip_scheduler_n_devices.restype = i
    L.schro_hip_scheduler_context.argtypes = [vp, i]
    L.schro_hip_scheduler_context.restype = vp
    L.schro_hip_scheduler_submit.argtypes = [vp, i, C.POINTER(C.c_int), i, i, PICTURE_FUNC, vp, C.POINTER(C.c_int)]
    L.schro_hip_scheduler_submit.restype = i
    L.schro_hip_scheduler_retire.argtypes = [vp, i]
    L.schro_hip_scheduler_retire.restype = i
    L.schro_hip_scheduler_wait.argtypes = [vp]
    L.schro_hip_scheduler_wait.restype = i
    L.schro_hip_context_select_queue.argtypes = [vp, i]
    L.schro_hip_context_select_queue.restype = i
    L.schro_hip_context_queue.argtypes = [vp]
    L.schro_hip_context_queue.restype = i
    L.schro_hip_queue_wait.argtypes = [vp, i, i]
    L.schro_hip_queue_wait.restype = i
    L.schro_hip_queue_mark.argtypes = [vp, i]
    L.schro_hip_queue_mark.restype = i
    L.schro_hip_queue_wait_mark.argtypes = [vp, i]
    L.schro_hip_queue_wait_mark.restype = i
    L.schro_hip_timer_begin.argtypes = [vp]
    L.schro_hip_timer_begin.restype = i
    L.schro_hip_timer_end.argtypes = [vp]
    L.schro_hip_timer_end.restype = C.c_float
    L.schro_hip_profile_enable.argtypes = [vp, i]
    L.schro_hip_profile_enable.restype = i
    L.schro_hip_profile_reset.argtypes = [vp]
    L.schro_hip_profile_reset.restype = i
    L.schro_hip_profile_read.argtypes = [vp, i, C.POINTER(C.c_double), C.POINTER(C.c_int)]
    L.schro_hip_profile_read.restype = i
    L.schro_hip_obmc_routes.argtypes = [vp, C.POINTER(C.c_longlong), i]
    L.schro_hip_obmc_routes.restype = i
    L.schro_hip_v210_routes.argtypes = [vp, C.POINTER(C.c_longlong), i]
    L.schro_hip_v210_routes.restype = i
    L.schro_hip_pack8_routes.argtypes = [vp, C.POINTER(C.c_longlong), i]
    L.schro_hip_pack8_routes.restype = i
    L.schro_hip_wide_routes.argtypes = [vp, C.POINTER(C.c_longlong), i]
    L.schro_hip_wide_routes.restype = i
    L.schro_hip_unpack_routes.argtypes = [vp, C.POINTER(C.c_longlong), i]
    L.schro_hip_unpack_routes.restype = i
    L.schro_hip_unpack_batch.argtypes = [vp, C.POINTER(UnpackPicture), i]
    L.schro_hip_unpack_batch.restype = i
    L.schro_hip_unpack_iwt_batch.argtypes = [vp, C.POINTER(UnpackIwtPicture), i, i, i, i]
    L.schro_hip_unpack_iwt_batch.restype = i
    L.schro_hip_iiwt_batch.argtypes = [vp, C.POINTER(IwtPlane), i, i, i, i]
    L.schro_hip_iiwt_batch.restype = i
    L.schro_hip_iwt_batch.argtypes = [vp, C.POINTER(IwtFwdPlane), i, i, i, i]
    L.schro_hip_iwt_batch.restype = i
    L.schro_hipframe_iwt_transform.argtypes = [vp, C.POINTER(Frame), C.POINTER(Params)]
    L.schro_hipframe_iwt_transform.restype = i
    L.schro_hip_downsample_batch.argtypes = [vp, C.POINTER(DownsamplePlane), i]
    L.schro_hip_downsample_batch.restype = i
    L.schro_hip_metric_scan_setup.argtypes = [C.POINTER(MetricScan), i, i, i, i, i, i]
    L.schro_hip_metric_scan_setup.restype = i
    L.schro_hip_metric_scan_batch.argtypes = [vp, C.POINTER(MetricScanPicture), i]
    L.schro_hip_metric_scan_batch.restype = i
    L.schro_hipframe_downsample.argtypes = [C.POINTER(Frame), C.POINTER(Frame)]
    L.schro_hipframe_downsample.restype = i
    L.schro_rough_me_heirarchical_scan_nohint_hip.argtypes = [C.POINTER(Frame), C.POINTER(Frame), C.POINTER(Params), i, i, i, vp]
    L.schro_rough_me_heirarchical_scan_nohint_hip.restype = i
    L.schro_hip_rough_hint_batch.argtypes = [vp, C.POINTER(RoughHintPicture), i]
    L.schro_hip_rough_hint_batch.restype = i
    L.schro_hip_rough_me_batch.argtypes = [vp, C.POINTER(RoughChain), i, i, i]
    L.schro_hip_rough_me_batch.restype = i
    L.schro_hip_rough_hint_check.argtypes = [C.POINTER(RoughHintPicture), i]
    L.schro_hip_rough_hint_check.restype = i
    L.schro_hip_rough_me_check.argtypes = [C.POINTER(RoughChain), i, i, i]
    L.schro_hip_rough_me_check.restype = i
    L.schro_rough_me_heirarchical_scan_hint_hip.argtypes = [C.POINTER(Frame), C.POINTER(Frame), C.POINTER(Params), i, i, i, vp, vp]
    L.schro_rough_me_heirarchical_scan_hint_hip.restype = i
    L.schro_rough_me_heirarchical_scan_hip.argtypes = [C.POINTER(C.POINTER(Frame)), C.POINTER(C.POINTER(Frame)), C.POINTER(Params), i, i,
                                                       C.POINTER(vp)]
    L.schro_rough_me_heirarchical_scan_hip.restype = i
    L.schro_hip_hbm_level_batch.argtypes = [vp, C.POINTER(HbmLevel), i]
    L.schro_hip_hbm_level_batch.restype = i
    L.schro_hip_hbm_batch.argtypes = [vp, C.POINTER(HbmChain), i, i]
    L.schro_hip_hbm_batch.restype = i
    L.schro_hip_hbm_level_check.argtypes = [C.POINTER(HbmLevel), i]
    L.schro_hip_hbm_level_check.restype = i
    L.schro_hip_hbm_check.argtypes = [C.POINTER(HbmChain), i, i]
    L.schro_hip_hbm_check.restype = i
    L.schro_hierarchical_bm_scan_hint_hip.argtypes = [C.POINTER(Frame), C.POINTER(Frame), C.POINTER(Params), i, i, i, vp, vp]
    L.schro_hierarchical_bm_scan_hint_hip.restype = i
    L.schro_hbm_scan_hip.argtypes = [C.POINTER(C.POINTER(Frame)), C.POINTER(C.POINTER(Frame)), C.POINTER(Params), i, i, i,
                                     C.POINTER(C.c_void_p)]
    L.schro_hbm_scan_hip.restype = i
    L.schro_hip_subpel_error_batch.argtypes = [vp, C.POINTER(SubpelChain), i, i, C.POINTER(C.c_void_p)]
    L.schro_hip_subpel_error_batch.restype = i
    L.schro_hip_subpel_choose_batch.argtypes = [vp, C.POINTER(SubpelChain), i, i, C.POINTER(C.c_void_p)]
    L.schro_hip_subpel_choose_batch.restype = i
    L.schro_hip_subpel_batch.argtypes = [vp, C.POINTER(SubpelChain), i]
    L.schro_hip_subpel_batch.restype = i
    L.schro_hip_subpel_check.argtypes = [C.POINTER(SubpelChain), i]
    L.schro_hip_subpel_check.restype = i
    L.schro_encoder_motion_predict_subpel_deep_hip.argtypes = [C.POINTER(Frame), C.POINTER(C.POINTER(Frame)), C.POINTER(Params), C.c_double,
                                                               C.POINTER(C.c_void_p)]
    L.schro_encoder_motion_predict_subpel_deep_hip.restype = i
    for name in ("schro_hip_split2_metric_batch", "schro_hip_split2_choose_batch"):
        getattr(L, name).argtypes = [vp, C.POINTER(Split2Picture), i, C.POINTER(C.c_void_p)]
        getattr(L, name).restype = i
    L.schro_hip_split2_batch.argtypes = [vp, C.POINTER(Split2Picture), i]
    L.schro_hip_split2_batch.restype = i
    L.schro_hip_split2_check.argtypes = [C.POINTER(Split2Picture), i]
    L.schro_hip_split2_check.restype = i
    L.schro_mode_decision_split2_hip.argtypes = [C.POINTER(Frame), C.POINTER(C.POINTER(Frame)), C.POINTER(Params), C.c_double,
                                                 C.POINTER(C.c_void_p), vp, vp]
    L.schro_mode_decision_split2_hip.restype = i
    for name in ("schro_hip_mode_metric_batch", "schro_hip_mode_choose_batch"):
        getattr(L, name).argtypes = [vp, C.POINTER(ModePicture), i, C.POINTER(C.c_void_p)]
        getattr(L, name).restype = i
    L.schro_hip_mode_decision_batch.argtypes = [vp, C.POINTER(ModePicture), i]
    L.schro_hip_mode_decision_batch.restype = i
    L.schro_hip_mode_decision_check.argtypes = [C.POINTER(ModePicture), i]
    L.schro_hip_mode_decision_check.restype = i
    L.schro_mode_decision_hip.argtypes = [C.POINTER(Frame), C.POINTER(C.POINTER(Frame)), C.POINTER(Params), C.c_double,
                                          C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), vp, vp, vp, C.POINTER(C.c_double)]
    L.schro_mode_decision_hip.restype = i
    L.schro_hip_convert_u8_batch.argtypes = [vp, C.POINTER(ConvertPlane), i, i]
    L.schro_hip_convert_u8_batch.restype = i
    L.schro_hip_upsample_batch.argtypes = [vp, C.POINTER(UpsamplePlane), i]
    L.schro_hip_upsample_batch.restype = i
    L.schro_hip_pack_u8_batch.argtypes = [vp, C.POINTER(PackPlane), i]
    L.schro_hip_pack_u8_batch.restype = i
    L.schro_hip_pack_v210_batch.argtypes = [vp, C.POINTER(PackPlane), i, i]
    L.schro_hip_pack_v210_batch.restype = i
    L.schro_hip_iiwt_pack_v210_batch.argtypes = [vp, C.POINTER(IwtPackPicture), i, i, i, i]
    L.schro_hip_iiwt_pack_v210_batch.restype = i
    L.schro_hip_iiwt_pack_u8_batch.argtypes = [vp, C.POINTER(IwtPack8Picture), i, i, i, i]
    L.schro_hip_iiwt_pack_u8_batch.restype = i
    L.schro_hip_iiwt_pack_wide_batch.argtypes = [vp, C.POINTER(IwtPackWidePicture), i, i, i, i]
    L.schro_hip_iiwt_pack_wide_batch.restype = i
    L.schro_hip_lowdelay_arith.argtypes = [C.POINTER(LowDelayParams), i]
    L.schro_hip_lowdelay_arith.restype = i
    L.schro_hip_lowdelay_batch.argtypes = [vp, C.POINTER(LowDelayPicture), i, C.POINTER(LowDelayParams), i]
    L.schro_hip_lowdelay_batch.restype = i
    L.schro_hip_decode_lowdelay_transform_data.argtypes = [C.POINTER(Frame), vp, C.c_size_t, C.POINTER(LowDelayParams)]
    L.schro_hip_decode_lowdelay_transform_data.restype = i
    L.schro_hip_lowdelay_encode_batch.argtypes = [vp, C.POINTER(LowDelayEncodePicture), i, C.POINTER(LowDelayParams), i]
    L.schro_hip_lowdelay_encode_batch.restype = i
    L.schro_hip_encode_lowdelay_transform_data.argtypes = [C.POINTER(Frame), vp, C.c_size_t, C.POINTER(LowDelayParams),
                                                           vp, C.POINTER(C.c_int)]
    L.schro_hip_encode_lowdelay_transform_data.restype = i
    L.schro_hip_noarith_encode_bound.argtypes = [C.POINTER(NoarithPicture), i]
    L.schro_hip_noarith_encode_bound.restype = C.c_int64
    L.schro_hip_noarith_encode_batch.argtypes = [vp, C.POINTER(NoarithPicture), i, i]
    L.schro_hip_noarith_encode_batch.restype = i
    L.schro_hip_noarith_encode_check.argtypes = [C.POINTER(NoarithPicture), i, i]
    L.schro_hip_noarith_encode_check.restype = i
    L.schro_hip_encode_transform_data_noarith.argtypes = [C.POINTER(Frame), C.POINTER(Params), C.POINTER(C.POINTER(C.c_int)), vp,
                                                          C.c_size_t, C.POINTER(C.c_size_t),
                                                          C.POINTER(C.c_int * NOARITH_MAX_SUBBANDS), C.POINTER(C.c_int)]
    L.schro_hip_encode_transform_data_noarith.restype = i
    L.schro_hip_noarith_decode_batch.argtypes = [vp, C.POINTER(NoarithDecodePicture), i, i]
    L.schro_hip_noarith_decode_batch.restype = i
    L.schro_hip_noarith_decode_check.argtypes = [C.POINTER(NoarithDecodePicture), i, i]
    L.schro_hip_noarith_decode_check.restype = i
    L.schro_hip_noarith_decode_scratch_words.argtypes = [C.POINTER(NoarithDecodePicture), i, i]
    L.schro_hip_noarith_decode_scratch_words.restype = C.c_int64
    L.schro_hipframe_decode_transform_data_noarith.argtypes = [C.POINTER(Frame), vp, C.c_size_t, C.POINTER(Params), C.POINTER(C.c_int),
                                                               C.POINTER(NoarithDecodeResult)]
    L.schro_hipframe_decode_transform_data_noarith.restype = i
    L.schro_hip_arith_decode_batch.argtypes = [vp, C.POINTER(ArithDecodePicture), i, i]
    L.schro_hip_arith_decode_batch.restype = i
    L.schro_hip_arith_decode_check.argtypes = [C.POINTER(ArithDecodePicture), i, i]
    L.schro_hip_arith_decode_check.restype = i
    L.schro_hip_arith_decode_scratch_words.argtypes = [C.POINTER(ArithDecodePicture), i, i]
    L.schro_hip_arith_decode_scratch_words.restype = C.c_int64
    L.schro_hipframe_decode_transform_data_arith.argtypes = [C.POINTER(Frame), vp, C.c_size_t, C.POINTER(Params), C.POINTER(C.c_int),
                                                             C.POINTER(ArithDecodeResult)]
    L.schro_hipframe_decode_transform_data_arith.restype = i
    L.schro_hip_motion_encode_bound.argtypes = [i, i, i, i]
    L.schro_hip_motion_encode_bound.restype = C.c_int64
    L.schro_hip_motion_encode_batch.argtypes = [vp, C.POINTER(MotionEncodePicture), i]
    L.schro_hip_motion_encode_batch.restype = i
    L.schro_hip_motion_encode_check.argtypes = [C.POINTER(MotionEncodePicture), i]
    L.schro_hip_motion_encode_check.restype = i
    L.schro_hip_encode_motion_data_noarith.argtypes = [vp, C.POINTER(Motion), C.POINTER(Params), vp, C.c_size_t,
                                                       C.POINTER(C.c_size_t), C.POINTER(C.c_int), C.POINTER(MotionEncodeResult)]
    L.schro_hip_encode_motion_data_noarith.restype = i
    L.schro_hip_motion_decode_batch.argtypes = [vp, C.POINTER(MotionDecodePicture), i]
    L.schro_hip_motion_decode_batch.restype = i
    L.schro_hip_motion_decode_check.argtypes = [C.POINTER(MotionDecodePicture), i]
    L.schro_hip_motion_decode_check.restype = i
    L.schro_hip_motion_decode_scratch_words.argtypes = [C.POINTER(MotionDecodePicture), i]
    L.schro_hip_motion_decode_scratch_words.restype = C.c_int64
    L.schro_hip_decode_motion_data_noarith.argtypes = [vp, vp, C.c_size_t, C.POINTER(Params), C.POINTER(Motion),
                                                       C.POINTER(MotionDecodeResult)]
    L.schro_hip_decode_motion_data_noarith.restype = i
    L.schro_hip_motion_arith_decode_batch.argtypes = [vp, C.POINTER(MotionArithDecodePicture), i]
    L.schro_hip_motion_arith_decode_batch.restype = i
    L.schro_hip_motion_arith_decode_check.argtypes = [C.POINTER(MotionArithDecodePicture), i]
    L.schro_hip_motion_arith_decode_check.restype = i
    L.schro_hip_motion_arith_decode_scratch_words.argtypes = [C.POINTER(MotionArithDecodePicture), i]
    L.schro_hip_motion_arith_decode_scratch_words.restype = C.c_int64
    L.schro_hip_decode_motion_data_arith.argtypes = [vp, vp, C.c_size_t, C.POINTER(Params), C.POINTER(Motion),
                                                     C.POINTER(MotionArithDecodeResult)]
    L.schro_hip_decode_motion_data_arith.restype = i
    L.schro_hip_dc_predict_batch.argtypes = [vp, C.POINTER(DcPlane), i, i]
    L.schro_hip_dc_predict_batch.restype = i
    L.schro_hip_shift_right_batch.argtypes = [vp, C.POINTER(DcPlane), i, i, i]
    L.schro_hip_shift_right_batch.restype = i
    L.schro_hip_pack_wide_batch.argtypes = [vp, C.POINTER(PackPlane), i, i]
    L.schro_hip_pack_wide_batch.restype = i
    L.schro_hipframe_shift_right.argtypes = [C.POINTER(Frame), i]
    L.schro_hipframe_shift_right.restype = i
    L.schro_hip_add_batch.argtypes = [vp, C.POINTER(ConvertPlane), i, i]
    L.schro_hip_add_batch.restype = i
    L.schro_hipframe_add.argtypes = [C.POINTER(Frame), C.POINTER(Frame)]
    L.schro_hipframe_add.restype = i
    L.schro_hip_dequant_batch.argtypes = [vp, C.POINTER(DequantPlane), i, i, i]
    L.schro_hip_dequant_batch.restype = i
    L.schro_hip_quantise_batch.argtypes = [vp, C.POINTER(QuantPlane), i, i]
    L.schro_hip_quantise_batch.restype = i
    L.schro_hip_subtract_batch.argtypes = [vp, C.POINTER(ConvertPlane), i, i]
    L.schro_hip_subtract_batch.restype = i
    L.schro_hipframe_subtract.argtypes = [C.POINTER(Frame), C.POINTER(Frame)]
    L.schro_hipframe_subtract.restype = i
    L.schro_hipframe_quantise.argtypes = [C.POINTER(Frame), C.POINTER(Frame), C.POINTER(Params), C.POINTER(C.POINTER(C.c_int)),
                                          C.POINTER(C.POINTER(CodeblockSummary))]
    L.schro_hipframe_quantise.restype = i
    L.schro_hip_histogram_batch.argtypes = [vp, C.POINTER(HistogramPlane), i, i]
    L.schro_hip_histogram_batch.restype = i
    L.schro_hipframe_subband_histograms.argtypes = [C.POINTER(Frame), C.POINTER(Params), C.POINTER(Histogram), C.POINTER(C.c_uint32)]
    L.schro_hipframe_subband_histograms.restype = i
    dp = C.POINTER(C.c_double)
    L.schro_hip_quant_choose_tables.argtypes = [vp, dp, dp, dp]
    L.schro_hip_quant_choose_tables.restype = i
    L.schro_hip_quant_choose_batch.argtypes = [vp, C.POINTER(QuantChoosePicture), i]
    L.schro_hip_quant_choose_batch.restype = i
    L.schro_hip_quant_choose_check.argtypes = [C.POINTER(QuantChoosePicture), i, i]
    L.schro_hip_quant_choose_check.restype = i
    L.schro_hip_quantise_chosen_batch.argtypes = [vp, C.POINTER(QuantPlane), C.POINTER(C.c_void_p), i, i, vp]
    L.schro_hip_quantise_chosen_batch.restype = i
    L.schro_hip_noarith_encode_chosen_batch.argtypes = [vp, C.POINTER(NoarithPicture), C.POINTER(C.c_void_p), i, i, vp]
    L.schro_hip_noarith_encode_chosen_batch.restype = i
    L.schro_hip_noarith_encode_chosen_check.argtypes = [C.POINTER(NoarithPicture), C.POINTER(C.c_void_p), i, i, vp]
    L.schro_hip_noarith_encode_chosen_check.restype = i
    L.schro_encoder_choose_quantisers_hip.argtypes = [C.POINTER(Frame), C.POINTER(Params), C.POINTER(QuantChooseSettings), vp]
    L.schro_encoder_choose_quantisers_hip.restype = i
    L.schro_hip_upsampled_bytes.argtypes = [i, i, C.POINTER(C.c_int)]
    L.schro_hip_upsampled_bytes.restype = C.c_size_t
    L.schro_hip_upsampled_download.argtypes = [vp, vp, i, vp, i, i, i]
    L.schro_hip_upsampled_download.restype = i
    L.schro_hip_upsampled_pair_bytes.argtypes = [i, i, C.POINTER(C.c_int)]
    L.schro_hip_upsampled_pair_bytes.restype = C.c_size_t
    L.schro_hip_upsampled_pair_download.argtypes = [vp, vp, vp, i, vp, i, i, i]
    L.schro_hip_upsampled_pair_download.restype = i
    L.schro_hip_obmc_batch.argtypes = [vp, C.POINTER(ObmcPlane), i]
    L.schro_hip_obmc_batch.restype = i
    L.schro_hip_obmc_prediction_epoch.argtypes = [vp]
    L.schro_hip_obmc_prediction_epoch.restype = C.c_uint
    L.schro_hip_obmc_overflowed.argtypes = [vp, C.POINTER(C.c_uint), i]
    L.schro_hip_obmc_overflowed.restype = i
    L.schro_hip_frame_new_and_alloc.argtypes = [vp, i, i, i, i]
    L.schro_hip_frame_new_and_alloc.restype = C.POINTER(Frame)
    L.schro_hip_frame_ref.argtypes = [C.POINTER(Frame)]
    L.schro_hip_frame_ref.restype = C.POINTER(Frame)
    L.schro_hip_frame_unref.argtypes = [C.POINTER(Frame)]
    L.schro_hip_frame_unref.restype = None
    L.schro_frame_to_hip.argtypes = [C.POINTER(Frame), C.POINTER(Frame)]
    L.schro_frame_to_hip.restype = i
    L.schro_hipframe_to_cpu.argtypes = [C.POINTER(Frame), C.POINTER(Frame)]
    L.schro_hipframe_to_cpu.restype = i
    L.schro_frame_inverse_iwt_transform_hip.argtypes = [C.POINTER(Frame), C.POINTER(Frame),
                                                        C.POINTER(Params)]
    L.schro_frame_inverse_iwt_transform_hip.restype = i
    L.schro_frame_inverse_iwt_transform_combine_hip.argtypes = [C.POINTER(Frame), C.POINTER(Frame),
                                                                 C.POINTER(Params), C.POINTER(Frame)]
    L.schro_frame_inverse_iwt_transform_combine_hip.restype = i
    L.schro_hipframe_dequantise.argtypes = [C.POINTER(Frame), C.POINTER(QuantisedPicture), C.POINTER(Params)]
    L.schro_hipframe_dequantise.restype = i
    L.schro_frame_inverse_iwt_transform_convert_hip.argtypes = [C.POINTER(Frame), C.POINTER(Frame), C.POINTER(Params)]
    L.schro_frame_inverse_iwt_transform_convert_hip.restype = i
    L.schro_frame_inverse_iwt_transform_combine_convert_hip.argtypes = [C.POINTER(Frame), C.POINTER(Frame), C.POINTER(Params),
                                                                        C.POINTER(Frame)]
    L.schro_frame_inverse_iwt_transform_combine_convert_hip.restype = i
    L.schro_frame_inverse_iwt_transform_shift_convert_hip.argtypes = [C.POINTER(Frame), C.POINTER(Frame), C.POINTER(Params), i]
    L.schro_frame_inverse_iwt_transform_shift_convert_hip.restype = i
    L.schro_upsampled_hipframe_upsample.argtypes = [C.POINTER(Frame), C.POINTER(Frame)]
    L.schro_upsampled_hipframe_upsample.restype = i
    L.schro_motion_render_hip.argtypes = [C.POINTER(Motion), C.POINTER(Frame), C.POINTER(Frame), i,
                                          C.POINTER(Frame)]
    L.schro_motion_render_hip.restype = i
    L.schro_hipframe_convert.argtypes = [C.POINTER(Frame), C.POINTER(Frame)]
    L.schro_hipframe_convert.restype = i
    L.schro_hipframe_convert_input.argtypes = [C.POINTER(Frame), C.POINTER(Frame)]
    L.schro_hipframe_convert_input.restype = i
    L.schro_hipframe_unpack_iwt_transform.argtypes = [C.POINTER(Frame), C.POINTER(Frame), C.POINTER(Params), i, i]
    L.schro_hipframe_unpack_iwt_transform.restype = i
    d = C.c_double
    L.schro_hip_plane_sums_batch.argtypes = [vp, C.POINTER(SumsJob), i]
    L.schro_hip_plane_sums_batch.restype = i
    L.schro_hip_plane_sums_check.argtypes = [C.POINTER(SumsJob), i]
    L.schro_hip_plane_sums_check.restype = i
    L.schro_hip_lowpass2_coeff.argtypes = [d, C.POINTER(d)]
    L.schro_hip_lowpass2_coeff.restype = None
    L.schro_hip_lowpass2_batch.argtypes = [vp, C.POINTER(Lowpass2Plane), i]
    L.schro_hip_lowpass2_batch.restype = i
    L.schro_hip_lowpass2_check.argtypes = [C.POINTER(Lowpass2Plane), i]
    L.schro_hip_lowpass2_check.restype = i
    L.schro_hip_ssim_scratch_bytes.argtypes = [i, i]
    L.schro_hip_ssim_scratch_bytes.restype = sz
    L.schro_hip_unpack_geometry.argtypes = [C.POINTER(i)]
    L.schro_hip_unpack_geometry.restype = None
    L.schro_hip_picture_stats_geometry.argtypes = [C.POINTER(i)]
    L.schro_hip_picture_stats_geometry.restype = None
    L.schro_hip_ssim_batch.argtypes = [vp, C.POINTER(SsimPicture), i]
    L.schro_hip_ssim_batch.restype = i
    L.schro_hip_ssim_check.argtypes = [C.POINTER(SsimPicture), i]
    L.schro_hip_ssim_check.restype = i
    L.schro_hipframe_calculate_average_luma.argtypes = [C.POINTER(Frame), C.POINTER(d)]
    L.schro_hipframe_calculate_average_luma.restype = i
    L.schro_hipframe_mean_squared_error.argtypes = [C.POINTER(Frame), C.POINTER(Frame), C.POINTER(d)]
    L.schro_hipframe_mean_squared_error.restype = i
    L.schro_hipframe_ssim.argtypes = [C.POINTER(Frame), C.POINTER(Frame), C.POINTER(d)]
    L.schro_hipframe_ssim.restype = i
    L.schro_hipframe_filter_lowpass2.argtypes = [C.POINTER(Frame), d]
    L.schro_hipframe_filter_lowpass2.restype = i
    L.schro_engine_get_scene_change_score_hip.argtypes = [C.POINTER(Frame), C.POINTER(Frame), d, C.POINTER(d)]
    L.schro_engine_get_scene_change_score_hip.restype = i
    _lib = L
    return L


class SchroHipError(RuntimeError):
    code = None         # the SCHRO_HIP_E* value where the error came from a call's return value


ENEEDS_RESIDUAL = -6    # SCHRO_HIP_ENEEDS_RESIDUAL: a routing answer of the combine form, not an error of the stream


def check(rc):
    if rc != 0:
        msg = load().schro_hip_last_error()
        e = SchroHipError("schro_hip error %d: %s" % (rc, msg.decode() if msg else "?"))
        e.code = rc
        raise e
