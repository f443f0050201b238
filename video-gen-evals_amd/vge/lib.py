"""ctypes binding of libvge.so (include/vge.h).  The product path has no fallback: if the HIP
library cannot be loaded every compute call raises VgeError."""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import numpy as np
import torch

_HERE = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ.get("VGE_LIB", _HERE / "libvge.so"))

VGE_OK = 0
STATUS = {0: "VGE_OK", 1: "VGE_ERR_ARG", 2: "VGE_ERR_HIP", 3: "VGE_ERR_MISSING_WEIGHT", 4: "VGE_ERR_WEIGHT_SHAPE",
          5: "VGE_ERR_NOMEM", 6: "VGE_ERR_WORKSPACE", 7: "VGE_ERR_UNSUPPORTED", 8: "VGE_ERR_DEVICE"}
VGE_ERR_UNSUPPORTED = 7
VGE_ERR_DEVICE = 8

EXPORTS = ["vge_featurize", "vge_featurize_layout", "vge_layout_feat_dim", "vge_stats_finalize_layout",
           "vge_encoder_feat_dim", "vge_stats_workspace_bytes", "vge_stats_accumulate", "vge_stats_finalize",
           "vge_encoder_create", "vge_encoder_reserve", "vge_encoder_destroy", "vge_encode", "vge_tc_windows",
           "vge_score_videos", "vge_centroid_accumulate", "vge_centroid_finalize", "vge_last_error", "vge_version",
           "vge_encoder_profile_begin", "vge_encoder_profile_read", "vge_encoder_profile_mask", "vge_encoder_wait_conv", "vge_ingest_probe",
           "vge_encoder_set_tail_stream", "vge_encoder_status", "vge_encoder_clear_status",
           "vge_ingest_decode",
           "vge_ingest_default_threads",
           "vge_ingest_probe_mem", "vge_ingest_decode_mem", "vge_ingest_plan_mem", "vge_ingest_decode_device",
           "vge_ingest_decode_device_workspace_bytes", "vge_ingest_decode_device_batch_symbols",
           "vge_ingest_decode_device_ring_bytes", "vge_ingest_decode_device_stage_bytes", "vge_inflate_check_lengths",
           "vge_hmr_create", "vge_hmr_reserve", "vge_hmr_destroy", "vge_hmr_extract", "vge_hmr_profile_begin",
           "vge_hmr_profile_read", "vge_op_gemm_bf16", "vge_op_gemm_lib", "vge_op_vit_attention", "vge_op_layernorm_bf16",
           "vge_op_patchify", "vge_op_xattn1", "vge_op_softmax_rows_bf16", "vge_op_hmr_readout",
           "vge_op_cast_rows_bf16", "vge_op_bcast_rows", "vge_op_copy_rows",
           "vge_dwpose_create", "vge_dwpose_reserve", "vge_dwpose_destroy", "vge_dwpose_keypoints",
           "vge_dwpose_profile_begin", "vge_dwpose_profile_read", "vge_op_conv_bf16",
           "vge_op_dwconv_bf16", "vge_op_spp_pool_bf16", "vge_op_chan_attn_bf16", "vge_op_upsample2x_bf16",
           "vge_op_warp_prep", "vge_op_letterbox_focus", "vge_op_head_scalenorm_t", "vge_op_scalenorm_rows",
           "vge_op_gau_attn", "vge_op_simcc_decode", "vge_op_yolox_decode_nms",
           "vge_yolox_create", "vge_yolox_reserve", "vge_yolox_destroy", "vge_yolox_detect", "vge_yolox_detect_scored",
           "vge_hmr_crop",
           "vge_yolox_profile_begin", "vge_yolox_profile_read",
           "vge_frcnn_create", "vge_frcnn_reserve", "vge_frcnn_destroy", "vge_frcnn_shapes", "vge_frcnn_detect",
           "vge_frcnn_profile_begin", "vge_frcnn_profile_read",
           "vge_op_frcnn_preprocess", "vge_op_frcnn_pool_s2", "vge_op_frcnn_stem_pool", "vge_op_rpn_proposals",
           "vge_op_roi_align", "vge_op_det_post",
           "vge_jpeg_probe", "vge_jpeg_make_layout", "vge_jpeg_entropy_decode", "vge_jpeg_reconstruct",
           "vge_jpeg_reconstruct_host",
           "vge_jpeg_quant_tables", "vge_jpeg_forward", "vge_jpeg_forward_host", "vge_jpeg_entropy_encode",
           "vge_jpeg_entropy_encode_mem", "vge_jpeg_write_files", "vge_jpeg_entropy_workspace_bytes",
           "vge_jpeg_entropy_plan", "vge_jpeg_entropy_emit", "vge_jpeg_entropy_segment_blocks",
           "vge_jpeg_file_sizes", "vge_jpeg_read_files",
           "vge_jpeg_probe_mem", "vge_jpeg_entropy_decode_mem", "vge_jpeg_entropy_decode_workspace_bytes",
           "vge_jpeg_entropy_decode_device", "vge_jpeg_entropy_decode_subsequence_bytes",
           "vge_jpeg_entropy_decode_tile_bytes",
           "vge_png_probe", "vge_png_probe_mem", "vge_png_decode", "vge_png_decode_mem", "vge_png_plan_mem",
           "vge_png_decode_device", "vge_png_decode_device_workspace_bytes", "vge_png_decode_device_band_rows",
           "vge_gif_probe", "vge_gif_probe_mem", "vge_gif_decode", "vge_gif_decode_mem", "vge_gif_plan_mem",
           "vge_gif_decode_device", "vge_gif_decode_device_workspace_bytes",
           "vge_webp_probe", "vge_webp_probe_mem", "vge_webp_decode", "vge_webp_decode_mem", "vge_webp_plan_mem",
           "vge_webp_decode_device", "vge_webp_decode_device_workspace_bytes", "vge_webp_slot_bytes",
           "vge_apng_probe", "vge_apng_probe_mem", "vge_apng_decode", "vge_apng_decode_mem", "vge_apng_plan_mem",
           "vge_apng_decode_device", "vge_apng_decode_device_workspace_bytes",
           "vge_time_gather", "vge_tcl_workspace_bytes", "vge_tcl_loss", "vge_hardneg_loss", "vge_centroid_distance",
           "vge_tcl_grad_workspace_bytes", "vge_tcl_loss_grad", "vge_hardneg_loss_grad",
           "vge_convblock_workspace_bytes", "vge_convblock_forward_workspace_bytes", "vge_convblock_forward", "vge_convblock_backward",
           "vge_timelayer_workspace_bytes", "vge_timelayer_forward_workspace_bytes", "vge_timelayer_forward",
           "vge_timelayer_backward",
           "vge_linear_workspace_bytes", "vge_linear_forward", "vge_linear_backward",
           "vge_fusion_workspace_bytes", "vge_fusion_forward_workspace_bytes", "vge_fusion_forward",
           "vge_fusion_backward"]


class VgeError(RuntimeError):
    pass


class UnsupportedModelError(VgeError):
    """VGE_ERR_UNSUPPORTED: a checkpoint whose d_model / time_heads / modality set the kernels are not built for
    (load_model, eval.py:136-165, would build such a HumanActionScorer; this library refuses it by name)."""


class DeviceFaultError(VgeError):
    """VGE_ERR_DEVICE: a kernel raised the encoder's status word (a broken invariant, e.g. the conv kernel's
    half-workgroup exchange wait ran out): the results of that launch are wrong and must not be used."""


class Dims(C.Structure):
    _fields_ = [("n_modalities", C.c_int), ("dims_raw", C.c_int * 8), ("dims_diff", C.c_int * 8),
                ("d_model", C.c_int), ("time_layers", C.c_int), ("time_heads", C.c_int), ("clip_len", C.c_int)]


class TensorView(C.Structure):
    _fields_ = [("name", C.c_char_p), ("data", C.c_void_p), ("ndim", C.c_int), ("shape", C.c_int64 * 4)]


class ClipInfo(C.Structure):  # include/vge_ingest.h vge_clip_info
    _fields_ = [("n_frames", C.c_int32), ("vit_dim", C.c_int32), ("kp_frames", C.c_int32), ("status", C.c_int32)]


class InflateDesc(C.Structure):  # include/vge_ingest.h vge_inflate_desc
    _fields_ = [("src_off", C.c_int64), ("csize", C.c_int64), ("count", C.c_int64), ("dst_off", C.c_int64),
                ("ws_off", C.c_int64), ("method", C.c_int32), ("skip", C.c_int32), ("itemsize", C.c_int32),
                ("array", C.c_int32), ("video", C.c_int32), ("reserved", C.c_int32)]


INGEST_STATUS = {0: "OK", 1: "ERR_ARG", 2: "ERR_HIP", 7: "ERR_IO", 8: "ERR_SHAPE", 9: "ERR_KP"}


class JpegInfo(C.Structure):  # include/vge_frames.h vge_jpeg_info
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("n_comp", C.c_int32), ("h0", C.c_int32),
                ("v0", C.c_int32), ("status", C.c_int32)]


class JpegLayout(C.Structure):  # include/vge_frames.h vge_jpeg_layout
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("n_comp", C.c_int32), ("h0", C.c_int32),
                ("v0", C.c_int32), ("mcus_x", C.c_int32), ("mcus_y", C.c_int32), ("bw", C.c_int32 * 3),
                ("bh", C.c_int32 * 3), ("off", C.c_int32 * 3), ("blocks_per_frame", C.c_int32)]


JPEG_STATUS = {0: "OK", 1: "ERR_ARG", 2: "ERR_HIP", 7: "ERR_IO", 8: "ERR_SHAPE", 20: "ERR_PROGRESSIVE",
               21: "ERR_ARITHMETIC", 22: "ERR_PRECISION", 23: "ERR_COMPONENTS", 24: "ERR_SAMPLING"}
JPEG_UNSUPPORTED = {20: "progressive (or another non-baseline process)", 21: "arithmetic-coded", 22: "not 8-bit",
                    23: "neither 1 nor 3 components", 24: "sampling other than 4:4:4 / 4:2:2 / 4:2:0"}


class PngInfo(C.Structure):  # include/vge_png.h vge_png_info
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("color_type", C.c_int32), ("bit_depth", C.c_int32),
                ("interlace", C.c_int32), ("n_idat", C.c_int32), ("idat_bytes", C.c_int64), ("status", C.c_int32),
                ("reserved", C.c_int32)]


class PngDesc(C.Structure):  # include/vge_png.h vge_png_desc
    _fields_ = [("file_off", C.c_int64), ("file_bytes", C.c_int64), ("gat_off", C.c_int64), ("gat_bytes", C.c_int64),
                ("slot_off", C.c_int64), ("raw_bytes", C.c_int64), ("color_type", C.c_int32), ("frame", C.c_int32)]


class PngSegment(C.Structure):  # include/vge_png.h vge_png_segment
    _fields_ = [("src_off", C.c_int64), ("dst_off", C.c_int64), ("bytes", C.c_int64), ("desc", C.c_int32),
                ("reserved", C.c_int32)]


PNG_STATUS = {0: "OK", 1: "ERR_ARG", 2: "ERR_HIP", 7: "ERR_IO", 8: "ERR_SHAPE", 30: "ERR_INTERLACED",
              31: "ERR_BITDEPTH", 32: "ERR_PALETTE"}
PNG_UNSUPPORTED = {30: "interlaced", 31: "not 8 bits per sample", 32: "palette"}


class GifInfo(C.Structure):  # include/vge_gif.h vge_gif_info
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("n_frames", C.c_int32), ("status", C.c_int32),
                ("lzw_bytes", C.c_int64), ("n_blocks", C.c_int64)]


class GifDesc(C.Structure):  # include/vge_gif.h vge_gif_desc
    _fields_ = [("file_off", C.c_int64), ("file_bytes", C.c_int64), ("gat_off", C.c_int64), ("gat_bytes", C.c_int64),
                ("slot_off", C.c_int64), ("ct_off", C.c_int64), ("ct_size", C.c_int32), ("file", C.c_int32),
                ("index", C.c_int32), ("frame", C.c_int32), ("x", C.c_int32), ("y", C.c_int32), ("w", C.c_int32),
                ("h", C.c_int32), ("interlace", C.c_int32), ("min_code_size", C.c_int32), ("transparent", C.c_int32),
                ("disposal", C.c_int32), ("fill_rgb", C.c_int32), ("first_rgb", C.c_int32),
                ("plan_status", C.c_int32), ("reserved", C.c_int32)]


GifSegment = PngSegment  # include/vge_gif.h vge_gif_segment: the same shape

GIF_STATUS = {0: "OK", 1: "ERR_ARG", 2: "ERR_HIP", 7: "ERR_IO", 8: "ERR_SHAPE", 40: "ERR_NO_PALETTE",
              41: "ERR_BOUNDS"}
GIF_UNSUPPORTED = {40: "a frame without any colour table", 41: "a frame that reaches outside the logical screen"}


class WebpInfo(C.Structure):  # include/vge_webp.h vge_webp_info
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("n_frames", C.c_int32), ("status", C.c_int32),
                ("vp8l_bytes", C.c_int64), ("n_chunks", C.c_int64)]


class WebpDesc(C.Structure):  # include/vge_webp.h vge_webp_desc
    _fields_ = [("file_off", C.c_int64), ("file_bytes", C.c_int64), ("pay_off", C.c_int64), ("pay_bytes", C.c_int64),
                ("slot_off", C.c_int64), ("file", C.c_int32), ("index", C.c_int32), ("frame", C.c_int32),
                ("x", C.c_int32), ("y", C.c_int32), ("w", C.c_int32), ("h", C.c_int32), ("blend", C.c_int32),
                ("dispose", C.c_int32), ("key", C.c_int32), ("plan_status", C.c_int32), ("reserved", C.c_int32)]


WEBP_STATUS = {0: "OK", 1: "ERR_ARG", 2: "ERR_HIP", 7: "ERR_IO", 8: "ERR_SHAPE", 50: "ERR_LOSSY", 51: "ERR_BOUNDS",
               52: "ERR_GROUPS"}
WEBP_UNSUPPORTED = {50: "a lossy (VP8 / ALPH) frame",
                    51: "a frame outside the canvas, or of another size than its VP8L header",
                    52: "more prefix-code groups than the table arena holds"}
WEBP_MAX_GROUPS = 256   # include/vge_webp.h VGE_WEBP_MAX_GROUPS


class ApngInfo(C.Structure):  # include/vge_apng.h vge_apng_info
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("color_type", C.c_int32), ("bit_depth", C.c_int32),
                ("interlace", C.c_int32), ("n_frames", C.c_int32), ("default_image", C.c_int32), ("status", C.c_int32),
                ("n_chunks", C.c_int64), ("data_bytes", C.c_int64)]


class ApngDesc(C.Structure):  # include/vge_apng.h vge_apng_desc
    _fields_ = [("file_off", C.c_int64), ("file_bytes", C.c_int64), ("gat_off", C.c_int64), ("gat_bytes", C.c_int64),
                ("slot_off", C.c_int64), ("raw_bytes", C.c_int64), ("file", C.c_int32), ("index", C.c_int32),
                ("frame", C.c_int32), ("x", C.c_int32), ("y", C.c_int32), ("w", C.c_int32), ("h", C.c_int32),
                ("color_type", C.c_int32), ("dispose_op", C.c_int32), ("blend_op", C.c_int32), ("trns", C.c_int32),
                ("plan_status", C.c_int32)]


ApngSegment = PngSegment  # include/vge_apng.h vge_apng_segment: the same shape

APNG_STATUS = {0: "OK", 1: "ERR_ARG", 2: "ERR_HIP", 7: "ERR_IO", 8: "ERR_SHAPE", 30: "ERR_INTERLACED",
               31: "ERR_BITDEPTH", 32: "ERR_PALETTE", 60: "ERR_BOUNDS"}
APNG_UNSUPPORTED = PNG_UNSUPPORTED   # the kinds the still path refuses by name, in the same words


class FrameStoreC(C.Structure):
    _fields_ = [("pose", C.c_void_p), ("gori", C.c_void_p), ("betas", C.c_void_p), ("vit", C.c_void_p),
                ("kp", C.c_void_p), ("videos", C.c_void_p), ("n_videos", C.c_int)]


_lib = None


def load() -> C.CDLL:
    """Load libvge.so once; raise VgeError (no CPU fallback) when it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise VgeError(f"libvge.so not found at {LIB_PATH}: build it with `make -C video-gen-evals_amd/csrc` "
                       "(or __graft_entry__.build()); there is no CPU fallback")
    lib = C.CDLL(str(LIB_PATH))
    vp, i32, i64p = C.c_void_p, C.c_int, C.POINTER(C.c_int64)
    sig = {
        "vge_featurize": [C.POINTER(FrameStoreC), vp, i32, vp, vp, vp, vp],
        "vge_featurize_layout": [C.POINTER(FrameStoreC), vp, i32, vp, vp, i32, vp, vp],
        "vge_layout_feat_dim": [i32],
        "vge_stats_finalize_layout": [vp, i64p, i32, vp, vp, vp],
        "vge_encoder_feat_dim": [vp],
        "vge_stats_workspace_bytes": [i32],
        "vge_stats_accumulate": [C.POINTER(FrameStoreC), vp, vp, i32, vp, i64p, vp, C.c_size_t, vp],
        "vge_stats_finalize": [vp, i64p, vp, vp, vp],
        "vge_encoder_create": [C.POINTER(Dims), C.POINTER(TensorView), i32, i32, C.POINTER(vp)],
        "vge_encoder_reserve": [vp, i32],
        "vge_encoder_destroy": [vp],
        "vge_encode": [vp, vp, i32, i32, vp, vp, vp, vp],
        "vge_tc_windows": [vp, i32, i32, i32, vp, vp],
        "vge_score_videos": [vp, vp, vp, vp, vp, i32, i32, vp, vp, vp],
        "vge_centroid_accumulate": [vp, vp, i32, i32, i32, vp, vp, vp],
        "vge_centroid_finalize": [vp, vp, i32, i32, vp, vp],
        "vge_encoder_profile_begin": [vp, i32],
        "vge_encoder_wait_conv": [vp, vp],
        "vge_encoder_set_tail_stream": [vp, vp],
        "vge_encoder_profile_mask": [vp, i32],
        "vge_encoder_profile_read": [vp, C.POINTER(C.c_double), C.POINTER(C.c_int)],
        "vge_encoder_status": [vp],
        "vge_encoder_clear_status": [vp],
        "vge_last_error": [],
        "vge_version": [],
        "vge_ingest_probe": [C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), i32, i32, C.POINTER(ClipInfo)],
        "vge_ingest_decode": [C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), i32, i32, vp, i32, vp, vp, vp, vp, vp,
                              vp],
        "vge_ingest_probe_mem": [vp, C.c_int64, vp, vp, i32, i32, C.POINTER(ClipInfo)],
        "vge_ingest_decode_mem": [vp, C.c_int64, vp, vp, i32, i32, vp, i32, vp, vp, vp, vp, vp, vp],
        "vge_ingest_plan_mem": [vp, C.c_int64, vp, vp, i32, i32, vp, i32, C.POINTER(InflateDesc), C.POINTER(ClipInfo),
                                i64p],
        "vge_ingest_decode_device": [vp, C.c_int64, vp, i32, i32, C.c_int64, C.c_int64, i32, vp, vp, vp, vp, vp, vp,
                                     C.c_int64, vp, vp],
        "vge_ingest_decode_device_workspace_bytes": [C.POINTER(InflateDesc), i32],
        "vge_ingest_decode_device_batch_symbols": [],
        "vge_ingest_decode_device_ring_bytes": [],
        "vge_ingest_decode_device_stage_bytes": [],
        "vge_inflate_check_lengths": [vp, i32, i32],
        "vge_jpeg_probe": [C.POINTER(C.c_char_p), i32, i32, C.POINTER(JpegInfo)],
        "vge_jpeg_make_layout": [i32, i32, i32, i32, i32, C.POINTER(JpegLayout)],
        "vge_jpeg_entropy_decode": [C.POINTER(C.c_char_p), i32, i32, C.POINTER(JpegLayout), vp, vp, vp],
        "vge_jpeg_reconstruct": [vp, vp, C.POINTER(JpegLayout), i32, vp, vp],
        "vge_jpeg_reconstruct_host": [vp, vp, C.POINTER(JpegLayout), i32, i32, vp],
        "vge_jpeg_quant_tables": [i32, vp],
        "vge_jpeg_forward": [vp, C.POINTER(JpegLayout), i32, vp, vp, vp],
        "vge_jpeg_forward_host": [vp, C.POINTER(JpegLayout), i32, i32, vp, vp],
        "vge_jpeg_entropy_encode": [vp, vp, C.POINTER(JpegLayout), i32, i32, C.POINTER(C.c_char_p), vp, vp],
        "vge_jpeg_entropy_encode_mem": [vp, vp, C.POINTER(JpegLayout), i32, i32, vp, vp, C.c_int64, vp, vp],
        "vge_jpeg_write_files": [vp, vp, vp, i32, i32, C.POINTER(C.c_char_p), vp],
        "vge_jpeg_entropy_workspace_bytes": [C.POINTER(JpegLayout), i32],
        "vge_jpeg_entropy_plan": [vp, C.POINTER(JpegLayout), i32, vp, vp, vp, vp],
        "vge_jpeg_entropy_emit": [vp, vp, C.POINTER(JpegLayout), i32, vp, vp, C.c_int64, vp],
        "vge_jpeg_entropy_segment_blocks": [],
        "vge_jpeg_file_sizes": [C.POINTER(C.c_char_p), i32, i32, vp],
        "vge_jpeg_read_files": [C.POINTER(C.c_char_p), i32, i32, vp, vp, vp, C.c_int64, vp],
        "vge_jpeg_probe_mem": [vp, C.c_int64, vp, vp, i32, i32, C.POINTER(JpegInfo)],
        "vge_jpeg_entropy_decode_mem": [vp, C.c_int64, vp, vp, i32, i32, C.POINTER(JpegLayout), vp, vp, vp],
        "vge_jpeg_entropy_decode_workspace_bytes": [C.POINTER(JpegLayout), i32, C.c_int64],
        "vge_jpeg_entropy_decode_device": [vp, C.c_int64, vp, vp, i32, C.POINTER(JpegLayout), vp, vp, vp, vp, vp, vp],
        "vge_jpeg_entropy_decode_subsequence_bytes": [],
        "vge_jpeg_entropy_decode_tile_bytes": [],
        "vge_png_probe": [C.POINTER(C.c_char_p), i32, i32, C.POINTER(PngInfo)],
        "vge_png_probe_mem": [vp, C.c_int64, vp, vp, i32, i32, C.POINTER(PngInfo)],
        "vge_png_decode": [C.POINTER(C.c_char_p), i32, i32, i32, i32, i32, vp, vp],
        "vge_png_decode_mem": [vp, C.c_int64, vp, vp, i32, i32, i32, i32, i32, vp, vp],
        "vge_png_plan_mem": [vp, C.c_int64, vp, vp, i32, i32, i32, i32, i32, C.POINTER(PngDesc),
                             C.POINTER(PngSegment), C.c_int64, i64p, vp, i64p],
        "vge_png_decode_device": [vp, C.c_int64, vp, i32, vp, C.c_int64, i32, i32, i32, i32, vp, C.c_int64, vp, vp,
                                  vp],
        "vge_png_decode_device_workspace_bytes": [C.POINTER(PngDesc), i32],
        "vge_png_decode_device_band_rows": [],
        "vge_gif_probe": [C.POINTER(C.c_char_p), i32, i32, C.POINTER(GifInfo)],
        "vge_gif_probe_mem": [vp, C.c_int64, vp, vp, i32, i32, C.POINTER(GifInfo)],
        "vge_gif_decode": [C.POINTER(C.c_char_p), i32, i32, i32, i32, C.c_int64, vp, vp, vp, i64p],
        "vge_gif_decode_mem": [vp, C.c_int64, vp, vp, i32, i32, i32, i32, C.c_int64, vp, vp, vp, i64p],
        "vge_gif_plan_mem": [vp, C.c_int64, vp, vp, i32, i32, i32, i32, C.POINTER(GifDesc), C.c_int64, i64p,
                             C.POINTER(GifSegment), C.c_int64, i64p, vp, vp, i64p],
        "vge_gif_decode_device": [vp, C.c_int64, vp, i32, vp, C.c_int64, i32, i32, i32, i32, vp, C.c_int64, vp, vp,
                                  vp],
        "vge_gif_decode_device_workspace_bytes": [C.POINTER(GifDesc), i32],
        "vge_apng_probe": [C.POINTER(C.c_char_p), i32, i32, C.POINTER(ApngInfo)],
        "vge_apng_probe_mem": [vp, C.c_int64, vp, vp, i32, i32, C.POINTER(ApngInfo)],
        "vge_apng_decode": [C.POINTER(C.c_char_p), i32, i32, i32, i32, i32, C.c_int64, vp, vp, vp, i64p],
        "vge_apng_decode_mem": [vp, C.c_int64, vp, vp, i32, i32, i32, i32, i32, C.c_int64, vp, vp, vp, i64p],
        "vge_apng_plan_mem": [vp, C.c_int64, vp, vp, i32, i32, i32, i32, i32, C.POINTER(ApngDesc), C.c_int64, i64p,
                              C.POINTER(ApngSegment), C.c_int64, i64p, vp, vp, i64p],
        "vge_apng_decode_device": [vp, C.c_int64, vp, i32, vp, C.c_int64, i32, i32, i32, i32, i32, vp, C.c_int64, vp,
                                   vp, vp],
        "vge_apng_decode_device_workspace_bytes": [C.POINTER(ApngDesc), i32],
        "vge_webp_probe": [C.POINTER(C.c_char_p), i32, i32, C.POINTER(WebpInfo)],
        "vge_webp_probe_mem": [vp, C.c_int64, vp, vp, i32, i32, C.POINTER(WebpInfo)],
        "vge_webp_decode": [C.POINTER(C.c_char_p), i32, i32, i32, i32, C.c_int64, vp, vp, vp, i64p],
        "vge_webp_decode_mem": [vp, C.c_int64, vp, vp, i32, i32, i32, i32, C.c_int64, vp, vp, vp, i64p],
        "vge_webp_plan_mem": [vp, C.c_int64, vp, vp, i32, i32, i32, i32, C.POINTER(WebpDesc), C.c_int64, i64p, vp, vp,
                              i64p],
        "vge_webp_decode_device": [vp, C.c_int64, vp, i32, i32, i32, i32, i32, vp, C.c_int64, vp, vp, vp],
        "vge_webp_decode_device_workspace_bytes": [C.POINTER(WebpDesc), i32],
        "vge_webp_slot_bytes": [i32, i32],
        "vge_time_gather": [vp, vp, i32, i32, i32, vp, vp],
        "vge_tcl_workspace_bytes": [i32],
        "vge_tcl_loss": [vp, vp, i32, i32, C.c_double, C.c_double, C.c_double, vp, C.c_size_t, vp, vp],
        "vge_hardneg_loss": [vp, vp, i32, i32, C.c_double, vp, vp],
        "vge_centroid_distance": [vp, vp, vp, i32, i32, i32, vp, vp],
        "vge_tcl_grad_workspace_bytes": [i32],
        "vge_tcl_loss_grad": [vp, vp, i32, i32, C.c_double, C.c_double, C.c_double, vp, C.c_size_t, vp, vp, vp],
        "vge_hardneg_loss_grad": [vp, vp, i32, i32, C.c_double, vp, vp, vp, vp],
        "vge_convblock_workspace_bytes": [i32, i32, i32],
        "vge_convblock_forward_workspace_bytes": [i32],
        "vge_convblock_forward": [vp] * 6 + [i32] * 4 + [vp] * 6 + [C.c_size_t, vp],
        "vge_convblock_backward": [vp] * 10 + [i32] * 4 + [vp] * 6 + [C.c_size_t, vp],
        "vge_timelayer_workspace_bytes": [i32] * 5,
        "vge_timelayer_forward_workspace_bytes": [i32] * 5,
        "vge_timelayer_forward": [vp] * 17 + [i32] * 5 + [vp] * 7 + [C.c_size_t, vp],
        "vge_timelayer_backward": [vp] * 18 + [i32] * 5 + [vp] * 14 + [C.c_size_t, vp],
        "vge_linear_workspace_bytes": [i32] * 3,
        "vge_linear_forward": [vp, i32, vp, vp, i32, i32, i32, vp],
        "vge_linear_backward": [vp, vp, i32, vp, vp, vp, vp, C.c_size_t, i32, i32, i32, vp],
        "vge_fusion_workspace_bytes": [i32] * 3,
        "vge_fusion_forward_workspace_bytes": [i32] * 3,
        "vge_fusion_forward": [vp] * 13 + [i32] * 3 + [vp] * 6 + [C.c_size_t, vp],
        "vge_fusion_backward": [vp] * 18 + [i32] * 3 + [vp] * 13 + [C.c_size_t, vp],
    }
    for name, args in sig.items():
        f = getattr(lib, name)
        f.argtypes = args
        f.restype = C.c_int
    lib.vge_stats_workspace_bytes.restype = C.c_size_t
    lib.vge_tcl_workspace_bytes.restype = C.c_size_t
    lib.vge_tcl_grad_workspace_bytes.restype = C.c_size_t
    lib.vge_convblock_workspace_bytes.restype = C.c_size_t
    lib.vge_convblock_forward_workspace_bytes.restype = C.c_size_t
    lib.vge_timelayer_workspace_bytes.restype = C.c_size_t
    lib.vge_timelayer_forward_workspace_bytes.restype = C.c_size_t
    lib.vge_linear_workspace_bytes.restype = C.c_size_t
    lib.vge_fusion_workspace_bytes.restype = C.c_size_t
    lib.vge_fusion_forward_workspace_bytes.restype = C.c_size_t
    lib.vge_jpeg_entropy_workspace_bytes.restype = C.c_size_t
    lib.vge_jpeg_entropy_decode_workspace_bytes.restype = C.c_size_t
    lib.vge_ingest_decode_device_workspace_bytes.restype = C.c_size_t
    lib.vge_png_decode_device_workspace_bytes.restype = C.c_size_t
    lib.vge_gif_decode_device_workspace_bytes.restype = C.c_size_t
    lib.vge_webp_decode_device_workspace_bytes.restype = C.c_size_t
    lib.vge_apng_decode_device_workspace_bytes.restype = C.c_size_t
    lib.vge_webp_slot_bytes.restype = C.c_int64
    lib.vge_last_error.restype = C.c_char_p
    lib.vge_version.restype = C.c_char_p
    _lib = lib
    return lib


def check(status: int, what: str) -> None:
    if status != VGE_OK:
        msg = load().vge_last_error().decode(errors="replace")
        cls = {VGE_ERR_UNSUPPORTED: UnsupportedModelError, VGE_ERR_DEVICE: DeviceFaultError}.get(status, VgeError)
        raise cls(f"{what} failed: {STATUS.get(status, status)}: {msg}")


def bind(lib: C.CDLL, tag: str, sig: dict) -> C.CDLL:
    """Give the functions of `sig` (name -> argtypes) their argtypes and an int restype, once per library and tag."""
    flag = f"_{tag}_sig"
    if not getattr(lib, flag, False):
        for name, args in sig.items():
            f = getattr(lib, name)
            f.argtypes = args
            f.restype = C.c_int
        setattr(lib, flag, True)
    return lib


def tensor_views(state_dict):
    """state_dict -> (the float32 arrays the views point into, a TensorView array, its length): the weights argument
    of every vge_*_create.  The arrays must stay alive until the create call returns."""
    keep, views = [], []
    for k, v in state_dict.items():
        a = np.ascontiguousarray(np.asarray(v, dtype=np.float32))
        keep.append(a)
        tv = TensorView()
        tv.name = k.encode()
        tv.data = a.ctypes.data
        tv.ndim = a.ndim
        for i, s in enumerate(a.shape[:4]):
            tv.shape[i] = s
        views.append(tv)
    return keep, (TensorView * len(views))(*views), len(views)


class NativeModel:
    """Handle of a native extractor model, vge_<PREFIX>_{create, reserve, destroy, profile_begin, profile_read}: the
    weights resident in HBM plus a workspace that only grows.  A subclass sets PREFIX, calls _create from its __init__
    and adds its forward calls; .lib, .cfg, .device and .h (the C handle) are public."""
    PREFIX = ""

    def _call(self, fn: str, *args) -> None:
        name = f"vge_{self.PREFIX}_{fn}"
        check(getattr(self.lib, name)(*args), name)

    def _create(self, lib: C.CDLL, cfg, cfg_c: C.Structure, state_dict, device) -> None:
        self.lib, self.cfg, self.device = lib, cfg, torch.device(device)
        self.h, self._reserved = None, (0,)
        keep, arr, n = tensor_views(state_dict)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            self._call("create", C.byref(cfg_c), arr, n, C.byref(h))
        self.h = h

    def _reserve(self, n: int, *shape: int) -> None:
        """vge_<PREFIX>_reserve(h, n, *shape) when n exceeds what is reserved or `shape` (a frame size) changed."""
        if n > self._reserved[0] or shape != self._reserved[1:]:
            with torch.cuda.device(self.device):
                self._call("reserve", self.h, int(n), *shape)
            self._reserved = (n, *shape)

    def profile_begin(self, max_calls: int) -> None:
        self._call("profile_begin", self.h, int(max_calls))

    def _profile_read(self, stage_names, n_flops: int = 1):
        """({stage: summed ms over the recorded calls}, recorded calls, FLOPs per call: a float, or a tuple of n_flops)"""
        ms = (C.c_double * len(stage_names))()
        n = C.c_int()
        fl = (C.c_double * n_flops)()
        self._call("profile_read", self.h, ms, C.byref(n), fl)
        return dict(zip(stage_names, ms)), n.value, fl[0] if n_flops == 1 else tuple(fl)

    def close(self) -> None:
        if getattr(self, "h", None):
            self._call("destroy", self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
