"""ctypes binding of libffpic_hip.so (include/ffpic_hip.h).  Loading never touches
the GPU; compute entry points fail loudly (FfhipError) without a gfx950 device."""
import ctypes as C
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, os.environ.get("FFHIP_LIB") or "libffpic_hip.so")   # FFHIP_LIB: A/B runs of two builds in one gpurun call (tests/tools/ab_*.sh)
CSRC = os.path.join(HERE, "csrc")

# every symbol include/ffpic_hip.h declares (tests check the library exports them all)
EXPORTS = [
    "ffhip_device_count", "ffhip_init", "ffhip_shutdown", "ffhip_strerror", "ffhip_arch_name",
    "ffhip_malloc", "ffhip_free", "ffhip_memcpy_h2d", "ffhip_memcpy_d2h", "ffhip_memset",
    "ffhip_stream_create", "ffhip_stream_destroy", "ffhip_stream_sync",
    "ffhip_event_create", "ffhip_event_destroy", "ffhip_event_record", "ffhip_event_elapsed_ms",
    "hip_accl_init", "hip_accl_uninit", "ffhip_accl_ops_get",
    "ffhip_get_dct_ops", "ffhip_get_cs_ops", "ffhip_idct_4x4_hevc",
    "ffhip_jpeg_recon_batch", "ffhip_jpeg_workspace_bytes", "ffhip_jpeg_recon_batch_host",
    "ffhip_jpeg_kernel_name", "ffhip_copy_calibrate", "ffhip_jpeg_pattern_calibrate",
    "ffhip_yuv420_to_bgra", "ffhip_yuv420_to_bgra_16", "ffhip_yuv400_to_bgra_16",
    "ffhip_vp8_residual_batch", "ffhip_hevc_residual_batch", "ffhip_vp8_predict_recon",
    "ffhip_hevc_intra_recon", "ffhip_hevc_intra_plan", "ffhip_debug_hevc_plan_result", "ffhip_vp8_decode_frames_form", "ffhip_debug_huff_times", "ffhip_hevc_intra_recon_tiles", "ffhip_hevc_decode_tiles", "ffhip_vp8_loopfilter",
    "ffhip_jpeg_probe", "ffhip_jpeg_entropy_decode", "ffhip_jpeg_entropy_decode_mt", "ffhip_jpeg_entropy_batch", "ffhip_bmp_write",
    "ffhip_heif_grid_parse", "ffhip_heif_grid_compose", "ffhip_hevc_picture_layout", "ffhip_jpeg_decode_files", "ffhip_jpeg_decode_files_device", "ffhip_jpeg_entropy_batch_gpu", "ffhip_jpeg_stage_scan_test", "ffhip_jpeg_stage_scan_raw_test", "ffhip_jpeg_lut_test", "ffhip_host_malloc", "ffhip_host_free",
    "ffhip_shard_range", "ffhip_comm_unique_id", "ffhip_comm_init_rank", "ffhip_comm_destroy", "ffhip_batch_close", "ffhip_batch_complete",
    "ffhip_bgra_checksum", "ffhip_vp8_filter_params", "ffhip_vp8_predict_loopfilter", "ffhip_reload_env", "ffhip_env_value_test", "ffhip_vp8_decode_frames", "ffhip_bgra_layout",
    "ffhip_jpeg_recon_items", "ffhip_jpeg_decode_files_mixed_device", "ffhip_vp8_decode_items",
    "ffhip_vp8_dequant_factors", "ffhip_webp_probe", "ffhip_webp_parse", "ffhip_webp_parse_batch", "ffhip_webp_parse_device", "ffhip_webp_decode_files_device", "ffhip_debug_webp_last_parts",
    "ffhip_webp_probe_ex", "ffhip_webp_parse_ex", "ffhip_webp_parse_device_ex", "ffhip_webp_decode_files_device_ex", "ffhip_webp_decode_files_tensor_ex",
    "ffhip_vp8_libwebp_residual_mb", "ffhip_webp_libwebp_color", "ffhip_debug_vp8_decode_items_libwebp", "ffhip_debug_vp8_upsample_color",
    "ffhip_bgra_to_tensor_items", "ffhip_jpeg_decode_files_tensor", "ffhip_webp_decode_files_tensor",
    "ffhip_resize_axis_taps", "ffhip_bgra_resize_items", "ffhip_jpeg_decode_files_tensor_resized", "ffhip_webp_decode_files_tensor_resized",
    "ffhip_jpeg_scaled_block", "ffhip_jpeg_scaled_size", "ffhip_jpeg_scaled_rect", "ffhip_jpeg_scale_choose", "ffhip_jpeg_scaled_wg_blocks",
    "ffhip_jpeg_recon_items_scaled", "ffhip_jpeg_decode_files_mixed_device_scaled", "ffhip_jpeg_decode_files_tensor_scaled",
    "ffhip_debug_tensor_last_parts",
    "ffhip_jpeg_exif_orientation", "ffhip_webp_exif_orientation", "ffhip_orient_size", "ffhip_orient_rect", "ffhip_orient_inverse",
    "ffhip_bgra_orient_items", "ffhip_jpeg_decode_files_tensor_oriented", "ffhip_webp_decode_files_tensor_oriented",
    "ffhip_debug_orient_last_items",
    "ffhip_jpeg_probe_any", "ffhip_jpeg_progressive_decode", "ffhip_jpeg_progressive_batch_gpu", "ffhip_jpeg_decode_files_mixed_device_ex",
    "ffhip_debug_progressive_last", "ffhip_jpeg_decode_files_tensor_ex",
    "ffhip_jpeg_libjpeg_block", "ffhip_jpeg_libjpeg_picture", "ffhip_jpeg_recon_items_libjpeg",
    "ffhip_inflate", "ffhip_png_probe", "ffhip_png_picture", "ffhip_png_exif_orientation", "ffhip_png_decode_files_device",
    "ffhip_png_decode_files_tensor", "ffhip_debug_png_last", "ffhip_debug_png_times",
    "ffhip_vp8l_probe", "ffhip_vp8l_read_info", "ffhip_vp8l_picture", "ffhip_vp8l_decode_files_device", "ffhip_vp8l_decode_files_tensor",
    "ffhip_debug_vp8l_last", "ffhip_debug_vp8l_times",
    "ffhip_webp_alpha_probe", "ffhip_webp_alpha_plane", "ffhip_debug_webp_alpha_last", "ffhip_debug_webp_alpha_times",
    "ffhip_debug_scratch_fill",
    "ffhip_bgra_to_tensor_items_alpha", "ffhip_bgra_resize_items_premultiplied",
    "ffhip_png_decode_files_tensor_alpha", "ffhip_vp8l_decode_files_tensor_alpha", "ffhip_webp_decode_files_tensor_alpha",
    "ffhip_inflate_streams_device", "ffhip_png_decode_files_device_ex", "ffhip_png_decode_files_tensor_ex", "ffhip_debug_png_inflate",
    "ffhip_jpeg_encode_tables", "ffhip_jpeg_encode_block", "ffhip_jpeg_encode_header", "ffhip_jpeg_encode_bound", "ffhip_jpeg_encode_picture",
    "ffhip_jpeg_fdct_items", "ffhip_jpeg_huff_encode_items", "ffhip_jpeg_encode_items",
    "ffhip_deflate", "ffhip_deflate_bound", "ffhip_deflate_code_lengths", "ffhip_png_filtered_size", "ffhip_png_filter_picture",
    "ffhip_png_encode_bound", "ffhip_png_encode_picture", "ffhip_deflate_streams_device", "ffhip_png_encode_items",
    "ffhip_vp8l_encode_bound", "ffhip_vp8l_encode_residual", "ffhip_vp8l_encode_picture", "ffhip_vp8l_encode_items",
    "ffhip_vp8_encode_quality_index", "ffhip_vp8_encode_bound", "ffhip_vp8_encode_planes", "ffhip_vp8_encode_mbs", "ffhip_vp8_encode_picture",
    "ffhip_vp8_encode_items",
]


FFHIP_EINVAL, FFHIP_ENOMEM, FFHIP_ENODEV, FFHIP_EIO = -22, -12, -19, -5     # include/ffpic_hip.h:34-37
FFHIP_JPEG_ACCEPT_PROGRESSIVE, FFHIP_JPEG_MAX_SCANS = 1, 128
FFHIP_JPEG_PIXELS_LIBJPEG = 0x10
FFHIP_WEBP_PIXELS_LIBWEBP = 0x10
FFHIP_WEBP_ALPHA = 0x20
FFHIP_PNG_INFLATE_DEVICE = 0x1
FFHIP_EWEBP_LOSSLESS, FFHIP_EWEBP_ANIMATION, FFHIP_EWEBP_INTER_FRAME = -1001, -1002, -1003
FFHIP_JPEG_ENC_444, FFHIP_JPEG_ENC_422, FFHIP_JPEG_ENC_420, FFHIP_JPEG_ENC_GREY = 0, 1, 2, 3
FFHIP_EJPEG_NOSPACE, FFHIP_EJPEG_RANGE = -1101, -1102
FFHIP_JPEG_ENC_HEADER_MAX = 640
FFHIP_DEFLATE_CHUNK = 16384
FFHIP_PNG_FILTER_ADAPTIVE = 5
FFHIP_EPNG_NOSPACE, FFHIP_EDEFLATE_NOSPACE = -1201, -1202
FFHIP_VP8L_ENC_SUBTRACT_GREEN, FFHIP_VP8L_ENC_PREDICT = 1, 2
FFHIP_VP8L_ENC_TILE_BITS, FFHIP_VP8L_ENC_CHUNK = 4, 4096
FFHIP_EVP8L_NOSPACE = -1301
FFHIP_EVP8_NOSPACE, FFHIP_EVP8_PARTITION = -1401, -1402


class FfhipError(RuntimeError):
    pass


class HeifGrid(C.Structure):
    """ffhip_heif_grid"""
    _fields_ = [("version", C.c_uint8), ("flags", C.c_uint8), ("rows", C.c_uint16), ("cols", C.c_uint16),
                ("output_width", C.c_uint32), ("output_height", C.c_uint32)]


class HevcLayout(C.Structure):
    """ffhip_hevc_layout"""
    _fields_ = [("height", C.c_int32), ("y_stride", C.c_int32), ("uv_stride", C.c_int32), ("size", C.c_int64), ("u_offset", C.c_int64),
                ("v_offset", C.c_int64), ("pitch", C.c_int32), ("ctbrows", C.c_int32), ("ctbcols", C.c_int32)]


class BatchRecord(C.Structure):
    """ffhip_batch_record"""
    _fields_ = [("rank", C.c_int32), ("status", C.c_int32), ("first", C.c_int64), ("count", C.c_int64), ("checksum", C.c_uint64)]


class Vp8FilterHeader(C.Structure):
    """ffhip_vp8_filter_header"""
    _fields_ = [("filter_type", C.c_uint8), ("loop_filter_level", C.c_uint8), ("sharpness_level", C.c_uint8),
                ("segmentation_enabled", C.c_uint8), ("segment_feature_mode", C.c_uint8), ("lf_update_value", C.c_int8 * 4),
                ("loop_filter_adj_enable", C.c_uint8), ("mode_ref_lf_delta0", C.c_int8), ("mb_mode_delta0", C.c_int8),
                ("nbr_partitions", C.c_uint8)]


class Vp8QuantHeader(C.Structure):
    """ffhip_vp8_quant_header"""
    _fields_ = [("y_ac_qi", C.c_uint8), ("y_dc_delta", C.c_int8), ("y2_dc_delta", C.c_int8), ("y2_ac_delta", C.c_int8),
                ("uv_dc_delta", C.c_int8), ("uv_ac_delta", C.c_int8), ("segmentation_enabled", C.c_uint8),
                ("update_mb_segmentation_map", C.c_uint8), ("quantizer_update_value", C.c_int8 * 4)]


class WebpInfo(C.Structure):
    """ffhip_webp_info"""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("mbcols", C.c_int32), ("mbrows", C.c_int32), ("filter_type", C.c_int32),
                ("nbr_partitions", C.c_int32), ("quant", (C.c_uint16 * 8) * 4), ("filters", C.c_uint8 * 24),
                ("quant_header", Vp8QuantHeader), ("filter_header", Vp8FilterHeader)]


class PngInfo(C.Structure):
    """ffhip_png_info"""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("bit_depth", C.c_int32), ("color_type", C.c_int32), ("interlace", C.c_int32),
                ("has_trns", C.c_int32), ("palette_size", C.c_int32), ("n_passes", C.c_int32), ("filtered_bytes", C.c_uint64),
                ("pass_rows", C.c_int32 * 7), ("pass_row_bytes", C.c_int32 * 7)]


class Vp8lInfo(C.Structure):
    """ffhip_vp8l_info"""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("has_alpha", C.c_int32), ("n_transforms", C.c_int32), ("transforms", C.c_int32 * 4),
                ("predictor_bits", C.c_int32), ("cross_bits", C.c_int32), ("palette_size", C.c_int32), ("pixels_per_word", C.c_int32),
                ("cache_bits", C.c_int32), ("has_meta", C.c_int32), ("residual_width", C.c_int32)]


class WebpParsed(C.Structure):
    """ffhip_webp_parsed: caller arrays (host) of one file and its header"""
    _fields_ = [("modes", C.c_void_p), ("levels", C.c_void_p), ("mbinfo", C.c_void_p), ("resmap", C.c_void_p), ("n_mb_cap", C.c_int64),
                ("info", WebpInfo)]


class JpegGeom(C.Structure):
    """ffhip_jpeg_geom"""
    _fields_ = [("mcu_cols", C.c_int32), ("mcu_rows", C.c_int32), ("ncomp", C.c_int32),
                ("h", C.c_int32), ("v", C.c_int32), ("qt_id", C.c_int32 * 3)]

    @property
    def width(self):
        return self.mcu_cols * 8 * self.h

    @property
    def height(self):
        return self.mcu_rows * 8 * self.v

    @property
    def y_blocks(self):
        return self.mcu_cols * self.mcu_rows * self.h * self.v

    @property
    def c_blocks(self):
        return self.mcu_cols * self.mcu_rows


class JpegItem(C.Structure):
    """ffhip_jpeg_item: one picture of an ffhip_jpeg_recon_items call (device pointers)"""
    _fields_ = [("geom", JpegGeom), ("d_coef_y", C.c_void_p), ("d_coef_u", C.c_void_p), ("d_coef_v", C.c_void_p),
                ("d_quant", C.c_void_p), ("d_bgra", C.c_void_p), ("pitch", C.c_int64)]


class Vp8Item(C.Structure):
    """ffhip_vp8_item: one key frame of an ffhip_vp8_decode_items call (device pointers; h_modes, quant and filters on the host)"""
    _fields_ = [("mbcols", C.c_int32), ("mbrows", C.c_int32), ("h_modes", C.c_void_p), ("d_modes", C.c_void_p),
                ("d_levels", C.c_void_p), ("d_mbinfo", C.c_void_p), ("quant", (C.c_uint16 * 8) * 4), ("d_residual", C.c_void_p),
                ("d_resmap", C.c_void_p), ("filter_type", C.c_int32), ("filters", C.c_uint8 * 24), ("d_bgra", C.c_void_p),
                ("pitch", C.c_int64)]


FFHIP_TENSOR_U8, FFHIP_TENSOR_F16, FFHIP_TENSOR_F32 = 0, 1, 2


class TensorFormat(C.Structure):
    """ffhip_tensor_format"""
    _fields_ = [("dtype", C.c_int32), ("bgr", C.c_int32), ("planar", C.c_int32), ("scale", C.c_float * 3), ("bias", C.c_float * 3)]


FFHIP_ALPHA_DROP, FFHIP_ALPHA_STRAIGHT, FFHIP_ALPHA_PREMULTIPLIED, FFHIP_ALPHA_OVER = 0, 1, 2, 3


class TensorAlpha(C.Structure):
    """ffhip_tensor_alpha: what the sink and the chain make of the alpha byte (background: B,G,R,unused)"""
    _fields_ = [("mode", C.c_int32), ("source_premultiplied", C.c_int32), ("background", C.c_uint8 * 4), ("alpha_scale", C.c_float),
                ("alpha_bias", C.c_float)]


class TensorItem(C.Structure):
    """ffhip_tensor_item: one picture of an ffhip_bgra_to_tensor_items call (device pointers; strides in elements)"""
    _fields_ = [("d_bgra", C.c_void_p), ("pitch", C.c_int64), ("x0", C.c_int32), ("y0", C.c_int32), ("width", C.c_int32),
                ("height", C.c_int32), ("d_out", C.c_void_p), ("row_stride", C.c_int64), ("plane_stride", C.c_int64)]


class TensorOut(C.Structure):
    """ffhip_tensor_out"""
    _fields_ = [("d_out", C.c_void_p), ("row_stride", C.c_int64), ("plane_stride", C.c_int64)]


class Rect(C.Structure):
    """ffhip_rect"""
    _fields_ = [("x0", C.c_int32), ("y0", C.c_int32), ("width", C.c_int32), ("height", C.c_int32)]


FFHIP_RESIZE_BILINEAR, FFHIP_RESIZE_ANTIALIAS = 0, 1
FFHIP_RESIZE_MAX_SIDE = 16384


class ResizeItem(C.Structure):
    """ffhip_resize_item: one picture of an ffhip_bgra_resize_items call (device pointers; pitches in bytes)"""
    _fields_ = [("d_src", C.c_void_p), ("src_pitch", C.c_int64), ("x0", C.c_int32), ("y0", C.c_int32), ("width", C.c_int32),
                ("height", C.c_int32), ("d_dst", C.c_void_p), ("dst_pitch", C.c_int64), ("out_width", C.c_int32), ("out_height", C.c_int32)]


class Size(C.Structure):
    """ffhip_size"""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32)]


class OrientItem(C.Structure):
    """ffhip_orient_item: one picture of an ffhip_bgra_orient_items call (device pointers; pitches in bytes; the STORED rectangle)"""
    _fields_ = [("d_src", C.c_void_p), ("src_pitch", C.c_int64), ("x0", C.c_int32), ("y0", C.c_int32), ("width", C.c_int32),
                ("height", C.c_int32), ("d_dst", C.c_void_p), ("dst_pitch", C.c_int64), ("orientation", C.c_int32)]


class JpegSource(C.Structure):
    """ffhip_jpeg_source: a uint8 picture by byte strides (channels 3 or 1), or a BGRA picture (channels 4)"""
    _fields_ = [("pixels", C.c_void_p), ("row_stride", C.c_int64), ("pixel_stride", C.c_int64), ("chan", C.c_int64 * 3),
                ("channels", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("reserved", C.c_int32)]


class JpegFdctItem(C.Structure):
    """ffhip_jpeg_fdct_item (device pointers)"""
    _fields_ = [("src", JpegSource), ("layout", C.c_int32), ("quality", C.c_int32), ("d_coef_y", C.c_void_p), ("d_coef_u", C.c_void_p),
                ("d_coef_v", C.c_void_p)]


class JpegHuffItem(C.Structure):
    """ffhip_jpeg_huff_item (device pointers)"""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("layout", C.c_int32), ("quality", C.c_int32), ("restart", C.c_int32),
                ("d_coef_y", C.c_void_p), ("d_coef_u", C.c_void_p), ("d_coef_v", C.c_void_p), ("d_out", C.c_void_p), ("cap", C.c_size_t)]


class JpegEncodeItem(C.Structure):
    """ffhip_jpeg_encode_item (device pointers)"""
    _fields_ = [("src", JpegSource), ("layout", C.c_int32), ("quality", C.c_int32), ("restart", C.c_int32), ("reserved", C.c_int32),
                ("d_out", C.c_void_p), ("cap", C.c_size_t)]


def jpeg_source(pixels, width, height, row_stride, pixel_stride, chan=(0, 0, 0), channels=3):
    s = JpegSource()
    s.pixels, s.width, s.height, s.row_stride, s.pixel_stride, s.channels = pixels, width, height, row_stride, pixel_stride, channels
    for k in range(3):
        s.chan[k] = chan[k] if k < len(chan) else 0
    return s


class PngSource(C.Structure):
    """ffhip_png_source: a uint8 picture of 1..4 channels by byte strides, chan[] in file order (grey, A / R, G, B, A)"""
    _fields_ = [("pixels", C.c_void_p), ("row_stride", C.c_int64), ("pixel_stride", C.c_int64), ("chan", C.c_int64 * 4),
                ("channels", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("reserved", C.c_int32)]


class PngEncodeItem(C.Structure):
    """ffhip_png_encode_item (device pointers)"""
    _fields_ = [("src", PngSource), ("filter", C.c_int32), ("reserved", C.c_int32), ("d_out", C.c_void_p), ("cap", C.c_size_t)]


class Vp8lEncodeItem(C.Structure):
    """ffhip_vp8l_encode_item (device pointers); its source is a PngSource"""
    _fields_ = [("src", PngSource), ("flags", C.c_int32), ("reserved", C.c_int32), ("d_out", C.c_void_p), ("cap", C.c_size_t)]


class Vp8EncodeItem(C.Structure):
    """ffhip_vp8_encode_item (device pointers); its source is a JpegSource of 1 or 3 channels"""
    _fields_ = [("src", JpegSource), ("quality", C.c_int32), ("filter", C.c_int32), ("d_out", C.c_void_p), ("cap", C.c_size_t)]


def png_source(pixels, width, height, row_stride, pixel_stride, chan, channels=None):
    s = PngSource()
    s.pixels, s.width, s.height, s.row_stride, s.pixel_stride = pixels, width, height, row_stride, pixel_stride
    s.channels = len(chan) if channels is None else channels
    for k in range(4):
        s.chan[k] = chan[k] if k < len(chan) else 0
    return s


def jpeg_geom(mcu_cols, mcu_rows, ncomp=3, h=2, v=2, qt_id=(0, 1, 1)):
    g = JpegGeom()
    g.mcu_cols, g.mcu_rows, g.ncomp, g.h, g.v = mcu_cols, mcu_rows, ncomp, h, v
    for i in range(3):
        g.qt_id[i] = qt_id[i]
    return g


class AcclOps(C.Structure):
    """struct ffhip_accl_ops == struct accl_ops (arch/accl.h:20-25)"""
    _fields_ = [("idct_4x4", C.CFUNCTYPE(None, C.c_void_p, C.c_int)),
                ("idct_8x8", C.CFUNCTYPE(None, C.c_void_p, C.c_int)),
                ("type", C.c_int),
                ("tqe_next", C.c_void_p), ("tqe_prev", C.c_void_p)]


class DctOps(C.Structure):
    _fields_ = [("bitdepth", C.c_int),
                ("idct_4x4", C.CFUNCTYPE(None, C.c_void_p, C.c_int)),
                ("idct_8x8", C.CFUNCTYPE(None, C.c_void_p, C.c_int)),
                ("fdct_4x4", C.c_void_p), ("fdct_8x8", C.c_void_p)]


class CsOps(C.Structure):
    _fields_ = [("YUV_to_BGRA32", C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_int, C.c_int)),
                ("YUV420_to_BGRA32", C.c_void_p)]


def build(force=False):
    """Compile libffpic_hip.so in-tree with hipcc for gfx950 (works without a GPU)."""
    if force:
        subprocess.check_call(["make", "-s", "-C", CSRC, "clean"])
    subprocess.check_call(["make", "-s", "-C", CSRC, "-j4"])


_lib = None


def lib():
    """The loaded library.  Raises FfhipError if it has not been built: there is no
    fallback implementation."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FfhipError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                         "(or make -C ffpic_amd/csrc); there is no CPU fallback")
    L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    vp, i64, sz = C.c_void_p, C.c_int64, C.c_size_t
    L.ffhip_device_count.restype = C.c_int
    L.ffhip_init.argtypes = [C.c_int]
    L.ffhip_strerror.argtypes = [C.c_int]
    L.ffhip_strerror.restype = C.c_char_p
    L.ffhip_arch_name.restype = C.c_char_p
    L.ffhip_malloc.argtypes = [sz]
    L.ffhip_malloc.restype = vp
    L.ffhip_free.argtypes = [vp]
    L.ffhip_memcpy_h2d.argtypes = [vp, vp, sz, vp]
    L.ffhip_memcpy_d2h.argtypes = [vp, vp, sz, vp]
    L.ffhip_memset.argtypes = [vp, C.c_int, sz, vp]
    L.ffhip_stream_create.restype = vp
    L.ffhip_stream_destroy.argtypes = [vp]
    L.ffhip_stream_sync.argtypes = [vp]
    L.ffhip_event_create.restype = vp
    L.ffhip_event_destroy.argtypes = [vp]
    L.ffhip_event_record.argtypes = [vp, vp]
    L.ffhip_event_elapsed_ms.argtypes = [vp, vp]
    L.ffhip_event_elapsed_ms.restype = C.c_float
    L.ffhip_accl_ops_get.restype = C.POINTER(AcclOps)
    L.ffhip_get_dct_ops.argtypes = [C.c_int]
    L.ffhip_get_dct_ops.restype = C.POINTER(DctOps)
    L.ffhip_get_cs_ops.argtypes = [C.c_int]
    L.ffhip_get_cs_ops.restype = C.POINTER(CsOps)
    L.ffhip_idct_4x4_hevc.argtypes = [vp, vp, C.c_int, C.c_bool]
    L.ffhip_idct_4x4_hevc.restype = None
    L.ffhip_jpeg_recon_batch.argtypes = [C.POINTER(JpegGeom), C.c_int, vp, vp, vp, vp, i64, vp, i64, i64, vp, sz, vp]
    L.ffhip_jpeg_workspace_bytes.argtypes = [C.POINTER(JpegGeom), C.c_int]
    L.ffhip_jpeg_workspace_bytes.restype = sz
    L.ffhip_jpeg_recon_batch_host.argtypes = [C.POINTER(JpegGeom), C.c_int, vp, vp, vp, vp, i64, vp, i64, i64]
    L.ffhip_jpeg_kernel_name.argtypes = [C.POINTER(JpegGeom)]
    L.ffhip_jpeg_kernel_name.restype = C.c_char_p
    L.ffhip_copy_calibrate.argtypes = [vp, vp, sz, vp]
    L.ffhip_jpeg_pattern_calibrate.argtypes = [C.POINTER(JpegGeom), C.c_int, vp, vp, vp, vp, i64, vp, i64, i64, vp]
    ci = C.c_int
    L.ffhip_yuv420_to_bgra.argtypes = [vp, ci, vp, vp, vp, ci, ci, ci, ci, ci, i64, i64, i64, vp]
    L.ffhip_yuv420_to_bgra_16.argtypes = [vp, ci, vp, vp, vp, ci, ci, ci, ci, ci, ci, i64, i64, i64, vp]
    L.ffhip_yuv400_to_bgra_16.argtypes = [vp, ci, vp, ci, ci, ci, ci, ci, i64, i64, vp]
    L.ffhip_vp8_residual_batch.argtypes = [C.c_longlong, vp, vp, vp, vp, vp]
    L.ffhip_hevc_residual_batch.argtypes = [ci, C.c_longlong, vp, vp, vp, ci, ci, vp, vp]
    L.ffhip_jpeg_probe.argtypes = [vp, sz, C.POINTER(JpegGeom), C.POINTER(ci), C.POINTER(ci)]
    L.ffhip_jpeg_entropy_decode.argtypes = [vp, sz, C.POINTER(JpegGeom), vp, vp, vp, vp]
    L.ffhip_jpeg_entropy_decode_mt.argtypes = [vp, sz, C.POINTER(JpegGeom), vp, vp, vp, vp, ci]
    L.ffhip_jpeg_entropy_batch.argtypes = [vp, vp, ci, ci, C.POINTER(JpegGeom), vp, vp, vp, vp, vp]
    L.ffhip_bmp_write.argtypes = [C.c_char_p, vp, ci, ci, i64]
    L.ffhip_host_malloc.argtypes = [sz]
    L.ffhip_host_malloc.restype = vp
    L.ffhip_host_free.argtypes = [vp]
    L.ffhip_host_free.restype = None
    L.ffhip_jpeg_entropy_batch_gpu.argtypes = [vp, vp, ci, ci, C.POINTER(JpegGeom), vp, vp, vp, vp, vp, vp]
    L.ffhip_jpeg_decode_files_device.argtypes = [vp, vp, ci, ci, C.POINTER(JpegGeom), vp, i64, i64, vp, vp]
    L.ffhip_jpeg_decode_files.argtypes = [vp, vp, ci, ci, ci, C.POINTER(JpegGeom), vp, i64, i64, vp]
    L.ffhip_jpeg_recon_items.argtypes = [C.POINTER(JpegItem), ci, vp]
    L.ffhip_vp8_decode_items.argtypes = [C.POINTER(Vp8Item), ci, vp]
    L.ffhip_jpeg_decode_files_mixed_device.argtypes = [vp, vp, ci, ci, vp, vp, C.POINTER(JpegGeom), vp, vp]
    L.ffhip_vp8_dequant_factors.argtypes = [C.POINTER(Vp8QuantHeader), vp]
    L.ffhip_webp_probe.argtypes = [vp, sz, C.POINTER(ci), C.POINTER(ci), C.POINTER(ci), C.POINTER(ci)]
    L.ffhip_webp_parse.argtypes = [vp, sz, C.POINTER(WebpParsed)]
    L.ffhip_webp_parse_batch.argtypes = [vp, vp, ci, ci, C.POINTER(WebpParsed), vp]
    L.ffhip_webp_parse_device.argtypes = [vp, vp, ci, C.POINTER(WebpParsed), vp, vp]
    L.ffhip_debug_webp_last_parts.argtypes = [vp]
    L.ffhip_webp_decode_files_device.argtypes = [vp, vp, ci, ci, vp, vp, C.POINTER(WebpInfo), vp, vp]
    L.ffhip_webp_probe_ex.argtypes = [vp, sz, C.c_uint, C.POINTER(ci), C.POINTER(ci), C.POINTER(ci), C.POINTER(ci)]
    L.ffhip_webp_parse_ex.argtypes = [vp, sz, C.c_uint, C.POINTER(WebpParsed)]
    L.ffhip_webp_parse_device_ex.argtypes = [vp, vp, ci, C.c_uint, C.POINTER(WebpParsed), vp, vp]
    L.ffhip_webp_decode_files_device_ex.argtypes = [vp, vp, ci, ci, vp, vp, vp, C.c_uint, C.POINTER(WebpInfo), vp, vp]
    L.ffhip_vp8_libwebp_residual_mb.argtypes = [vp, ci, vp, vp, C.POINTER(ci)]
    L.ffhip_webp_libwebp_color.argtypes = [vp, i64, vp, vp, i64, ci, ci, vp, i64]
    L.ffhip_debug_vp8_decode_items_libwebp.argtypes = [C.POINTER(Vp8Item), ci, C.POINTER(Size), vp]
    L.ffhip_debug_vp8_upsample_color.argtypes = [vp, vp, vp, ci, ci, ci, ci, ci, i64, i64, vp, i64, i64, vp]
    L.ffhip_hevc_picture_layout.argtypes = [ci, ci, ci, C.POINTER(HevcLayout)]
    L.ffhip_heif_grid_parse.argtypes = [vp, sz, C.POINTER(HeifGrid)]
    L.ffhip_heif_grid_compose.argtypes = [vp, i64, ci, ci, vp, i64, i64, ci, ci, ci, ci, vp]
    L.ffhip_hevc_intra_plan.argtypes = [vp, C.c_longlong, ci, ci, ci, ci, ci, vp, vp, vp]
    L.ffhip_debug_hevc_plan_result.argtypes = [vp]
    L.ffhip_hevc_intra_recon.argtypes = [vp, vp, C.c_longlong, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, ci, vp]
    L.ffhip_hevc_intra_recon_tiles.argtypes = [vp, vp, C.c_longlong, vp, ci, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, ci, vp]
    L.ffhip_hevc_decode_tiles.argtypes = [vp, vp, C.c_longlong, vp, ci, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, ci, vp, i64, vp]
    L.ffhip_vp8_loopfilter.argtypes = [ci, ci, ci, ci, vp, vp, vp, vp, vp, i64, i64, vp]
    L.ffhip_vp8_predict_recon.argtypes = [ci, ci, ci, vp, vp, vp, i64, vp, vp, vp, vp, i64, i64, vp]
    L.ffhip_vp8_predict_loopfilter.argtypes = [ci, ci, ci, vp, vp, vp, i64, vp, ci, vp, vp, vp, vp, i64, i64, vp]
    ll = C.c_longlong
    L.ffhip_shard_range.argtypes = [ll, ci, ci, C.POINTER(ll), C.POINTER(ll)]
    L.ffhip_comm_unique_id.argtypes = [vp]
    L.ffhip_comm_init_rank.argtypes = [vp, ci, ci]
    L.ffhip_comm_init_rank.restype = vp
    L.ffhip_comm_destroy.argtypes = [vp]
    L.ffhip_comm_destroy.restype = None
    L.ffhip_batch_close.argtypes = [vp, ci, ci, ll, ll, ci, C.c_uint64, C.POINTER(BatchRecord), vp]
    L.ffhip_batch_complete.argtypes = [C.POINTER(BatchRecord), ci, ll]
    L.ffhip_vp8_filter_params.argtypes = [C.POINTER(Vp8FilterHeader), vp, C.POINTER(ci)]
    L.ffhip_bgra_checksum.argtypes = [vp, i64, i64, ci, ci, ci, vp, vp]
    L.ffhip_vp8_decode_frames.argtypes = [ci, ci, ci, vp, vp, vp, i64, vp, ci, vp, vp, ci, i64, vp, vp, vp, i64, i64, vp]
    L.ffhip_bgra_layout.argtypes = [C.POINTER(JpegGeom), C.POINTER(i64), C.POINTER(i64)]
    L.ffhip_bgra_to_tensor_items.argtypes = [C.POINTER(TensorItem), ci, C.POINTER(TensorFormat), vp]
    L.ffhip_jpeg_decode_files_tensor.argtypes = [vp, vp, ci, ci, C.POINTER(TensorFormat), C.POINTER(TensorOut), C.POINTER(Rect),
                                                 C.POINTER(JpegGeom), vp, vp]
    L.ffhip_webp_decode_files_tensor.argtypes = [vp, vp, ci, ci, C.POINTER(TensorFormat), C.POINTER(TensorOut), C.POINTER(Rect),
                                                 C.POINTER(WebpInfo), vp, vp]
    L.ffhip_resize_axis_taps.argtypes = [ci, ci, ci, ci, C.POINTER(ci), C.POINTER(C.c_uint16), ci]
    L.ffhip_bgra_resize_items.argtypes = [C.POINTER(ResizeItem), ci, ci, vp]
    L.ffhip_jpeg_decode_files_tensor_resized.argtypes = [vp, vp, ci, ci, C.POINTER(TensorFormat), C.POINTER(TensorOut), C.POINTER(Rect),
                                                         C.POINTER(Size), ci, C.POINTER(JpegGeom), vp, vp]
    L.ffhip_webp_decode_files_tensor_resized.argtypes = [vp, vp, ci, ci, C.POINTER(TensorFormat), C.POINTER(TensorOut), C.POINTER(Rect),
                                                         C.POINTER(Size), ci, C.POINTER(WebpInfo), vp, vp]
    L.ffhip_jpeg_scaled_block.argtypes = [vp, vp, ci, vp]
    L.ffhip_jpeg_scaled_size.argtypes = [ci, ci, ci, C.POINTER(ci), C.POINTER(ci)]
    L.ffhip_jpeg_scaled_rect.argtypes = [ci, ci, ci, C.POINTER(Rect), C.POINTER(Rect)]
    L.ffhip_jpeg_scale_choose.argtypes = [ci, ci, ci, ci]
    L.ffhip_jpeg_recon_items_scaled.argtypes = [C.POINTER(JpegItem), C.POINTER(ci), ci, vp]
    L.ffhip_jpeg_decode_files_mixed_device_scaled.argtypes = [vp, vp, ci, ci, vp, vp, C.POINTER(ci), C.POINTER(JpegGeom), vp, vp]
    L.ffhip_jpeg_decode_files_tensor_scaled.argtypes = [vp, vp, ci, ci, C.POINTER(TensorFormat), C.POINTER(TensorOut), C.POINTER(Rect),
                                                        C.POINTER(Size), ci, C.POINTER(ci), C.POINTER(ci), C.POINTER(JpegGeom), vp, vp]
    L.ffhip_jpeg_exif_orientation.argtypes = [vp, sz, C.POINTER(ci)]
    L.ffhip_webp_exif_orientation.argtypes = [vp, sz, C.POINTER(ci)]
    L.ffhip_orient_size.argtypes = [ci, ci, ci, C.POINTER(ci), C.POINTER(ci)]
    L.ffhip_orient_rect.argtypes = [ci, ci, ci, C.POINTER(Rect), C.POINTER(Rect)]
    L.ffhip_orient_inverse.argtypes = [ci]
    L.ffhip_bgra_orient_items.argtypes = [C.POINTER(OrientItem), ci, vp]
    L.ffhip_jpeg_decode_files_tensor_oriented.argtypes = [vp, vp, ci, ci, C.POINTER(TensorFormat), C.POINTER(TensorOut), C.POINTER(Rect),
                                                          C.POINTER(Size), ci, C.POINTER(ci), C.POINTER(ci), C.POINTER(ci), C.POINTER(ci),
                                                          C.POINTER(JpegGeom), vp, vp]
    L.ffhip_webp_decode_files_tensor_oriented.argtypes = [vp, vp, ci, ci, C.POINTER(TensorFormat), C.POINTER(TensorOut), C.POINTER(Rect),
                                                          C.POINTER(Size), ci, C.POINTER(ci), C.POINTER(ci), C.POINTER(WebpInfo), vp, vp]
    L.ffhip_webp_decode_files_tensor_ex.argtypes = [vp, vp, ci, ci, C.POINTER(TensorFormat), C.POINTER(TensorOut), C.POINTER(Rect),
                                                    C.POINTER(Size), ci, C.POINTER(ci), C.POINTER(ci), C.c_uint, C.POINTER(WebpInfo), vp, vp]
    L.ffhip_jpeg_probe_any.argtypes = [vp, sz, C.POINTER(JpegGeom), C.POINTER(ci), C.POINTER(ci), C.POINTER(ci)]
    L.ffhip_jpeg_progressive_decode.argtypes = [vp, sz, C.POINTER(JpegGeom), vp, vp, vp, vp, ci]
    L.ffhip_jpeg_progressive_batch_gpu.argtypes = [vp, vp, ci, ci, C.POINTER(JpegGeom), vp, vp, vp, vp, ci, vp, vp]
    L.ffhip_jpeg_decode_files_mixed_device_ex.argtypes = [vp, vp, ci, ci, vp, vp, C.POINTER(ci), C.c_uint, C.POINTER(JpegGeom), vp, vp]
    L.ffhip_debug_progressive_last.argtypes = [C.POINTER(ci)]
    L.ffhip_jpeg_decode_files_tensor_ex.argtypes = [vp, vp, ci, ci, C.POINTER(TensorFormat), C.POINTER(TensorOut), C.POINTER(Rect),
                                                    C.POINTER(Size), ci, C.POINTER(ci), C.POINTER(ci), C.POINTER(ci), C.POINTER(ci), C.c_uint,
                                                    C.POINTER(JpegGeom), vp, vp]
    L.ffhip_jpeg_libjpeg_block.argtypes = [vp, vp, vp]
    L.ffhip_jpeg_libjpeg_picture.argtypes = [C.POINTER(JpegGeom), ci, ci, vp, vp, vp, vp, vp, C.c_int64]
    L.ffhip_jpeg_recon_items_libjpeg.argtypes = [C.POINTER(JpegItem), C.POINTER(Size), ci, vp]
    L.ffhip_inflate.argtypes = [vp, sz, vp, sz, C.POINTER(sz)]
    L.ffhip_png_probe.argtypes = [vp, sz, C.POINTER(PngInfo)]
    L.ffhip_png_picture.argtypes = [vp, sz, vp, i64]
    L.ffhip_png_exif_orientation.argtypes = [vp, sz, C.POINTER(ci)]
    L.ffhip_png_decode_files_device.argtypes = [vp, vp, ci, ci, vp, vp, C.POINTER(PngInfo), vp, vp]
    L.ffhip_png_decode_files_tensor.argtypes = [vp, vp, ci, ci, C.POINTER(TensorFormat), C.POINTER(TensorOut), C.POINTER(Rect),
                                                C.POINTER(Size), ci, C.POINTER(ci), C.POINTER(ci), C.c_uint, C.POINTER(PngInfo), vp, vp]
    L.ffhip_debug_png_last.argtypes = [C.POINTER(ci)]
    L.ffhip_debug_png_times.argtypes = [C.POINTER(C.c_double)]
    L.ffhip_vp8l_probe.argtypes = [vp, sz, C.POINTER(ci), C.POINTER(ci), C.POINTER(ci)]
    L.ffhip_vp8l_read_info.argtypes = [vp, sz, C.POINTER(Vp8lInfo)]
    L.ffhip_vp8l_picture.argtypes = [vp, sz, vp, i64]
    L.ffhip_vp8l_decode_files_device.argtypes = [vp, vp, ci, ci, vp, vp, C.POINTER(Vp8lInfo), vp, vp]
    L.ffhip_vp8l_decode_files_tensor.argtypes = [vp, vp, ci, ci, C.POINTER(TensorFormat), C.POINTER(TensorOut), C.POINTER(Rect),
                                                 C.POINTER(Size), ci, C.POINTER(ci), C.POINTER(ci), C.c_uint, C.POINTER(Vp8lInfo), vp, vp]
    L.ffhip_debug_vp8l_last.argtypes = [C.POINTER(ci)]
    L.ffhip_debug_vp8l_times.argtypes = [C.POINTER(C.c_double)]
    L.ffhip_webp_alpha_probe.argtypes = [vp, sz, C.POINTER(ci), C.POINTER(ci), C.POINTER(ci), C.POINTER(ci)]
    L.ffhip_webp_alpha_plane.argtypes = [vp, sz, vp, i64]
    L.ffhip_debug_webp_alpha_last.argtypes = [C.POINTER(ci)]
    L.ffhip_debug_webp_alpha_times.argtypes = [C.POINTER(C.c_double)]
    L.ffhip_bgra_to_tensor_items_alpha.argtypes = [C.POINTER(TensorItem), ci, C.POINTER(TensorFormat), C.POINTER(TensorAlpha), vp]
    L.ffhip_bgra_resize_items_premultiplied.argtypes = [C.POINTER(ResizeItem), ci, ci, vp]
    for name, info in (("png", PngInfo), ("vp8l", Vp8lInfo), ("webp", WebpInfo)):
        getattr(L, f"ffhip_{name}_decode_files_tensor_alpha").argtypes = [
            vp, vp, ci, ci, C.POINTER(TensorFormat), C.POINTER(TensorOut), C.POINTER(Rect), C.POINTER(Size), ci, C.POINTER(ci), C.POINTER(ci),
            C.c_uint, C.POINTER(TensorAlpha), C.POINTER(info), vp, vp]
    L.ffhip_inflate_streams_device.argtypes = [vp, vp, ci, vp, vp, vp, vp, vp]
    L.ffhip_png_decode_files_device_ex.argtypes = [vp, vp, ci, ci, vp, vp, C.POINTER(PngInfo), vp, C.c_uint, vp]
    L.ffhip_png_decode_files_tensor_ex.argtypes = [vp, vp, ci, ci, C.POINTER(TensorFormat), C.POINTER(TensorOut), C.POINTER(Rect), C.POINTER(Size), ci,
                                                   C.POINTER(ci), C.POINTER(ci), C.c_uint, C.POINTER(TensorAlpha), C.c_uint, C.POINTER(PngInfo), vp, vp]
    L.ffhip_debug_png_inflate.argtypes = [C.POINTER(C.c_double)]
    L.ffhip_jpeg_encode_tables.argtypes = [ci, vp]
    L.ffhip_jpeg_encode_block.argtypes = [vp, vp, vp]
    L.ffhip_jpeg_encode_header.argtypes = [ci, ci, ci, ci, ci, vp, sz, C.POINTER(sz)]
    L.ffhip_jpeg_encode_bound.argtypes = [ci, ci, ci, ci]
    L.ffhip_jpeg_encode_bound.restype = sz
    L.ffhip_jpeg_encode_picture.argtypes = [C.POINTER(JpegSource), ci, ci, ci, vp, sz, C.POINTER(sz)]
    L.ffhip_jpeg_fdct_items.argtypes = [C.POINTER(JpegFdctItem), ci, vp]
    L.ffhip_jpeg_huff_encode_items.argtypes = [C.POINTER(JpegHuffItem), ci, C.POINTER(sz), C.POINTER(ci), vp]
    L.ffhip_jpeg_encode_items.argtypes = [C.POINTER(JpegEncodeItem), ci, C.POINTER(sz), C.POINTER(ci), vp]
    L.ffhip_deflate.argtypes = [vp, sz, vp, sz, C.POINTER(sz)]
    L.ffhip_deflate_bound.argtypes = [sz]
    L.ffhip_deflate_bound.restype = sz
    L.ffhip_deflate_code_lengths.argtypes = [vp, ci, ci, vp]
    L.ffhip_png_filtered_size.argtypes = [ci, ci, ci]
    L.ffhip_png_filtered_size.restype = sz
    L.ffhip_png_filter_picture.argtypes = [C.POINTER(PngSource), ci, vp, sz, C.POINTER(sz)]
    L.ffhip_png_encode_bound.argtypes = [ci, ci, ci]
    L.ffhip_png_encode_bound.restype = sz
    L.ffhip_png_encode_picture.argtypes = [C.POINTER(PngSource), ci, vp, sz, C.POINTER(sz)]
    L.ffhip_deflate_streams_device.argtypes = [vp, vp, ci, vp, vp, vp, vp, vp]
    L.ffhip_png_encode_items.argtypes = [C.POINTER(PngEncodeItem), ci, C.POINTER(sz), C.POINTER(ci), vp]
    L.ffhip_vp8l_encode_bound.argtypes = [ci, ci]
    L.ffhip_vp8l_encode_bound.restype = sz
    L.ffhip_vp8l_encode_residual.argtypes = [C.POINTER(PngSource), ci, vp, vp]
    L.ffhip_vp8l_encode_picture.argtypes = [C.POINTER(PngSource), ci, vp, sz, C.POINTER(sz)]
    L.ffhip_vp8l_encode_items.argtypes = [C.POINTER(Vp8lEncodeItem), ci, C.POINTER(sz), C.POINTER(ci), vp]
    L.ffhip_vp8_encode_quality_index.argtypes = [ci]
    L.ffhip_vp8_encode_bound.argtypes = [ci, ci]
    L.ffhip_vp8_encode_bound.restype = sz
    L.ffhip_vp8_encode_planes.argtypes = [C.POINTER(JpegSource), vp, vp, vp]
    L.ffhip_vp8_encode_mbs.argtypes = [C.POINTER(JpegSource), ci, vp, vp, vp, vp, vp, vp]
    L.ffhip_vp8_encode_picture.argtypes = [C.POINTER(JpegSource), ci, ci, vp, sz, C.POINTER(sz)]
    L.ffhip_vp8_encode_items.argtypes = [C.POINTER(Vp8EncodeItem), ci, C.POINTER(sz), C.POINTER(ci), vp]
    for name in ("ffhip_inflate_upto", "ffhip_inflate_model"):    # exported, not in the public header (csrc/ffhip_png_internal.h)
        getattr(L, name).argtypes = [vp, sz, vp, sz, C.POINTER(sz), ci]
    L.ffhip_inflate_model_mode.argtypes = [vp, sz, vp, sz, C.POINTER(sz), ci, ci]
    L.ffhip_debug_scratch_fill.argtypes = [vp, ci, C.POINTER(C.c_uint64), C.POINTER(ci), ci]
    L.ffhip_env_value_test.argtypes = [C.c_char_p, vp, sz]
    L.ffhip_env_value_test.restype = C.c_long
    _lib = L
    return L


def reload_env():
    """The library reads its FFHIP_* switches once per process; after changing one in a live process, call this."""
    if _lib is not None:
        _lib.ffhip_reload_env()


def setenv(name, value):
    """Set (or, with None, remove) an FFHIP_* switch in this process and make the library read it again."""
    if value is None:
        os.environ.pop(name, None)
    else:
        os.environ[name] = str(value)
    reload_env()


def check(rc, what="ffhip call"):
    if rc != 0:
        raise FfhipError(f"{what} failed: {rc} ({lib().ffhip_strerror(rc).decode()})")


FFHIP_RETRIED = 1


def sync(stream=None):
    """ffhip_stream_sync: raises on an error code, returns the status otherwise -- 0, or FFHIP_RETRIED when the sync had to repeat a
    side-by-side VP8 call (outputs good; what the caller enqueued behind that call consumed the aborted run's and is stale)."""
    rc = lib().ffhip_stream_sync(stream)
    if rc < 0:
        check(rc, "ffhip_stream_sync")
    return rc


def require_device(device=0):
    """Bind to a gfx950 device or raise: the product path never degrades to the CPU."""
    L = lib()
    if L.ffhip_device_count() <= device:
        raise FfhipError("no HIP device visible: ffpic_amd needs an MI355X (gfx950); there is no CPU fallback")
    check(L.ffhip_init(device), f"ffhip_init({device})")
    return L
