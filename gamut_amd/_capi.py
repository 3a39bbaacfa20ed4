"""ctypes binding of libgamut_hip.so (include/gamut_hip.h).

The product path: there is NO CPU fallback.  If the HIP library is missing the
import fails loudly; if no GPU is present every compute entry point returns
GAMUT_HIP_ERR_NO_DEVICE / a HIP error and `check()` raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GAMUT_HIP_LIB") or os.path.join(_HERE, "lib", "libgamut_hip.so")

OK, ERR_INVALID_ARG, ERR_UNSUPPORTED, ERR_OUT_OF_MEMORY, ERR_HIP, ERR_DECODE, ERR_NO_DEVICE = range(7)


class GamutHipError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(f"gamut_hip status {status}: {message}")
        self.status = status


class JpegDesc(C.Structure):
    _fields_ = [("coeffs", C.c_void_p), ("max_zag", C.c_void_p), ("out", C.c_void_p), ("out_pitch", C.c_int64),
                ("width", C.c_int32), ("height", C.c_int32), ("scan_type", C.c_int32), ("out_comps", C.c_int32)]


class PngInfo(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("channels_in_file", C.c_int32), ("channels", C.c_int32), ("bits", C.c_int32),
                ("pixels_per_meter_x", C.c_float), ("pixels_per_meter_y", C.c_float), ("pixel_aspect_ratio", C.c_float)]


class QoiDesc(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("channels", C.c_uint8), ("colorspace", C.c_uint8)]


class JpegFrame(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("comps", C.c_int32), ("scan_type", C.c_int32),
                ("mcus_per_row", C.c_int32), ("mcus_per_col", C.c_int32), ("blocks_per_mcu", C.c_int32),
                ("coeffs", C.POINTER(C.c_int16)), ("max_zag", C.POINTER(C.c_uint8)),
                ("pixel_aspect_ratio", C.c_float), ("dpi_y", C.c_float)]


class BmpInfo(C.Structure):                                    # gamut_hip_bmp_info
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("bpp", C.c_int32), ("header_size", C.c_int32), ("compression", C.c_int32),
                ("channels_in_file", C.c_int32), ("top_down", C.c_int32), ("pixel_offset", C.c_int32), ("palette_size", C.c_int32),
                ("mask_r", C.c_uint32), ("mask_g", C.c_uint32), ("mask_b", C.c_uint32), ("mask_a", C.c_uint32),
                ("pixels_per_meter_x", C.c_float), ("pixels_per_meter_y", C.c_float), ("pixel_aspect_ratio", C.c_float)]


class GifInfo(C.Structure):                                    # gamut_hip_gif_info
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("layers", C.c_int32), ("is_gif89", C.c_int32),
                ("pixel_aspect_ratio", C.c_float), ("fps", C.c_float)]


class TgaInfo(C.Structure):                                    # gamut_hip_tga_info
    _fields_ = [(n, C.c_int32) for n in ("width", "height", "bpp", "image_type", "rle", "indexed", "rgb16", "channels_in_file", "bottom_up",
                                         "palette_start", "palette_len", "cmap_size", "data_offset", "detected")]


class QoixInfo(C.Structure):                                   # gamut_hip_qoix_info
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("version", C.c_int32), ("channels", C.c_int32), ("bitdepth", C.c_int32),
                ("colorspace", C.c_int32), ("compression", C.c_int32), ("pixel_aspect_ratio", C.c_float), ("resolution_y", C.c_float),
                ("orig", C.c_int32), ("pixel_type", C.c_int32), ("detected", C.c_int32)]


class QoixDesc(C.Structure):                                   # gamut_hip_qoix_desc
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("channels", C.c_int32), ("colorspace", C.c_int32), ("mode", C.c_int32),
                ("pixel_aspect_ratio", C.c_float), ("resolution_y", C.c_float)]


class SqzInfo(C.Structure):                                    # gamut_hip_sqz_info
    _fields_ = [(n, C.c_int32) for n in ("width", "height", "planes", "color_mode", "levels", "scan_order", "subsampling", "pixel_type", "detected")]


class SqzDesc(C.Structure):                                    # gamut_hip_sqz_desc
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("color_mode", C.c_int32), ("levels", C.c_int32), ("coeff_offset", C.c_int64)]


class SqzEncodeDesc(C.Structure):                              # gamut_hip_sqz_encode_desc
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("color_mode", C.c_int32), ("levels", C.c_int32), ("scan_order", C.c_int32),
                ("subsampling", C.c_int32), ("budget", C.c_int64)]


class ImageInfo(C.Structure):                                  # gamut_hip_image_info
    _fields_ = [("format", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("channels_in_file", C.c_int32), ("channels", C.c_int32)]


class InflateDesc(C.Structure):
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("src_len", C.c_uint32), ("dst_cap", C.c_uint32)]


class PngDesc(C.Structure):
    _fields_ = [("raw", C.c_void_p), ("out", C.c_void_p), ("raw_len", C.c_uint32), ("x", C.c_uint32), ("y", C.c_uint32),
                ("img_n", C.c_int32), ("out_n", C.c_int32), ("depth", C.c_int32), ("color", C.c_int32)]


# name -> (restype, argtypes); mirrors include/gamut_hip.h one to one
_vp, _i, _i64, _u32, _sz, _f = C.c_void_p, C.c_int, C.c_int64, C.c_uint32, C.c_size_t, C.c_float
_pi, _pf = C.POINTER(C.c_int), C.POINTER(C.c_float)
SIGNATURES = {
    "gamut_hip_version": (C.c_char_p, []),
    "gamut_hip_device_count": (_i, []),
    "gamut_hip_init": (_i, [_i]),
    "gamut_hip_shutdown": (None, []),
    "gamut_hip_last_error": (C.c_char_p, []),
    "gamut_hip_device_malloc": (_vp, [_sz]),
    "gamut_hip_device_free": (None, [_vp]),
    "gamut_hip_host_malloc_pinned": (_vp, [_sz]),
    "gamut_hip_host_free_pinned": (None, [_vp]),
    "gamut_hip_memcpy_h2d": (_i, [_vp, _vp, _sz, _vp]),
    "gamut_hip_memcpy_d2h": (_i, [_vp, _vp, _sz, _vp]),
    "gamut_hip_stream_create": (_vp, []),
    "gamut_hip_stream_destroy": (None, [_vp]),
    "gamut_hip_stream_synchronize": (_i, [_vp]),
    "gamut_hip_pixel_type_size": (_i, [_i]),
    "gamut_hip_scanlines_inter_type": (_i, [_i, _i]),
    "gamut_hip_scanlines_convert": (_i, [_i, _vp, _i, _i, _vp, _i, _i, _i]),
    "gamut_hip_scanlines_copy": (_i, [_i, _vp, _i, _vp, _i, _i, _i]),
    "gamut_hip_scanlines_convert_device": (_i, [_i, _vp, _i64, _i64, _i, _vp, _i64, _i64, _i, _i, _i, _vp]),
    "gamut_hip_jpeg_reconstruct_device": (_i, [C.POINTER(JpegDesc), _i, _vp]),
    "gamut_hip_jpeg_reconstruct_batch_device": (_i, [_vp, _i64, _vp, _i64, _vp, _i64, _i64, _i, _i, _i, _i, _i, _vp]),
    "gamut_hip_jpeg_decode_coeffs": (_i, [_vp, _sz, C.POINTER(JpegFrame)]),
    "gamut_hip_png_read_header": (_i, [_vp, _sz, C.POINTER(PngInfo)]),
    "gamut_hip_png_decode_batch_device": (_i, [C.POINTER(_vp), C.POINTER(_sz), _i, _i, _i, C.POINTER(_i64), _vp, C.POINTER(PngInfo), C.POINTER(_i), _i, _vp]),
    "gamut_hip_qoi_decode": (_vp, [_vp, _i, C.POINTER(QoiDesc), _i]),
    "gamut_hip_qoi_read_header": (_i, [_vp, _i, C.POINTER(QoiDesc)]),
    "gamut_hip_qoi_decode_batch_device": (_i, [C.POINTER(_vp), C.POINTER(_i), _i, _i, C.POINTER(_i64), _vp, C.POINTER(QoiDesc), C.POINTER(_i), _vp]),
    "gamut_hip_qoi_decode_resident_device": (_i, [_vp, _i64, C.POINTER(_i64), C.POINTER(_i), C.POINTER(QoiDesc), _i, _i, C.POINTER(_i64), _vp, _vp]),
    "gamut_hip_qoi_encode_bound": (_i64, [C.POINTER(QoiDesc)]),
    "gamut_hip_qoi_encode": (_vp, [_vp, C.POINTER(QoiDesc), _i, _pi]),
    "gamut_hip_qoi_encode_batch_device": (_i, [C.POINTER(_vp), C.POINTER(_i64), C.POINTER(QoiDesc), _i, C.POINTER(_i64), _vp, C.POINTER(_i64),
                                           C.POINTER(_i), _vp]),
    "gamut_hip_jpeg_encode_bound": (_i64, [_i, _i, _i, _i]),
    "gamut_hip_jpeg_encode": (_vp, [_vp, _i, _i, _i, _i, _i, _pi]),
    "gamut_hip_jpeg_write_to_func": (_i, [_vp, _vp, _i, _i, _i, _vp, _i, _i]),
    "gamut_hip_jpeg_encode_batch_device": (_i, [C.POINTER(_vp), C.POINTER(_i64), _pi, _pi, _pi, _pi, _i, C.POINTER(_i64), _vp,
                                            C.POINTER(_i64), _pi, _vp]),
    "gamut_hip_png_encode_bound": (_i64, [_i, _i, _i, _i]),
    "gamut_hip_png_write_to_mem": (_vp, [_vp, _i, _i, _i, _i, _pi, _i, _i, _i]),
    "gamut_hip_png_encode_batch_device": (_i, [C.POINTER(_vp), C.POINTER(_i64), _pi, _pi, _pi, _pi, _pi, _pi, _i, C.POINTER(_i64), _vp,
                                           C.POINTER(_i64), _pi, _vp]),
    "gamut_hip_bmp_read_header": (_i, [_vp, _sz, C.POINTER(BmpInfo)]),
    "gamut_hip_bmp_decode_batch_device": (_i, [C.POINTER(_vp), C.POINTER(_sz), _i, _i, C.POINTER(_i64), _vp, C.POINTER(BmpInfo), _pi, _vp]),
    "gamut_hip_bmp_last_decode_kernel_ms": (_f, []),
    "gamut_hip_bmp_encode_bound": (_i64, [_i, _i, _i]),
    "gamut_hip_bmp_encode_batch_device": (_i, [C.POINTER(_vp), C.POINTER(_i64), _pi, _pi, _pi, _pi, _pi, _i, C.POINTER(_i64), _vp,
                                           C.POINTER(_i64), _pi, _vp]),
    "gamut_hip_bmp_write_to_mem": (_vp, [_vp, _i, _i, _i, _i, _i, _i, _pi]),
    "gamut_hip_gif_read_header": (_i, [_vp, _sz, C.POINTER(GifInfo)]),
    "gamut_hip_gif_decode_batch_device": (_i, [C.POINTER(_vp), C.POINTER(_sz), _i, C.POINTER(_i64), C.POINTER(_i64), _vp, C.POINTER(GifInfo), _pi, _vp]),
    "gamut_hip_gif_last_decode_kernel_ms": (_f, []),
    "gamut_hip_gif_last_kernel_ms": (_f, [_i]),
    "gamut_hip_gif_encode_bound": (_i64, [_i, _i, _i]),
    "gamut_hip_gif_encode_batch_device": (_i, [C.POINTER(_vp), C.POINTER(_i64), C.POINTER(_i64), _pi, _pi, _pi, _pi, _pi, _pi, _i, C.POINTER(_i64), _vp,
                                           C.POINTER(_i64), _pi, _vp]),
    "gamut_hip_gif_write_to_mem": (_vp, [_vp, _i, _i64, _i, _i, _i, _i, _i, _i, _pi]),
    "gamut_hip_gif_last_encode_kernel_ms": (_f, [_i]),
    "gamut_hip_tga_read_header": (_i, [_vp, _sz, C.POINTER(TgaInfo)]),
    "gamut_hip_tga_decode_batch_device": (_i, [C.POINTER(_vp), C.POINTER(_sz), _i, _i, C.POINTER(_i64), _vp, C.POINTER(TgaInfo), _pi, _vp]),
    "gamut_hip_tga_rle_window": (_i, []),
    "gamut_hip_tga_last_decode_kernel_ms": (_f, []),
    "gamut_hip_tga_encode_bound": (_i64, [_i, _i, _i]),
    "gamut_hip_tga_encode_batch_device": (_i, [C.POINTER(_vp), C.POINTER(_i64), _pi, _pi, _pi, _pi, _i, C.POINTER(_i64), _vp,
                                           C.POINTER(_i64), _pi, _vp]),
    "gamut_hip_tga_write_to_mem": (_vp, [_vp, _i, _i, _i, _i, _i, _pi]),
    "gamut_hip_tga_encode_window": (_i, []),
    "gamut_hip_tga_last_encode_kernel_ms": (_f, []),
    "gamut_hip_tga_last_encode_stage_ms": (_f, [_i]),
    "gamut_hip_dds_encode_bound": (_i64, [_i, _i, _i]),
    "gamut_hip_dds_encode_batch_device": (_i, [C.POINTER(_vp), C.POINTER(_i64), _pi, _pi, _pi, _i, C.POINTER(_i64), _vp, C.POINTER(_i64), _pi, _vp]),
    "gamut_hip_bc7_encode_blocks_device": (_i, [_vp, _i64, _vp, _vp]),
    "gamut_hip_dds_write_to_mem": (_vp, [_vp, _i, _i, _i, _i, _pi]),
    "gamut_hip_dds_last_encode_kernel_ms": (_f, []),
    "gamut_hip_qoix_read_header": (_i, [_vp, _sz, C.POINTER(QoixInfo)]),
    "gamut_hip_qoix_decode_batch_device": (_i, [C.POINTER(_vp), C.POINTER(_sz), _i, _i, C.POINTER(_i64), _vp, C.POINTER(QoixInfo), _pi, _vp]),
    "gamut_hip_qoix_lz4_decode": (_vp, [_vp, _i, C.POINTER(QoixInfo), _i, _pi]),
    "gamut_hip_qoix_row_capacity": (_i, []),
    "gamut_hip_qoix_last_decode_kernel_ms": (_f, []),
    "gamut_hip_qoix_last_decode_stage_ms": (_f, [_i]),
    "gamut_hip_qoix_set_plane": (_i, [_i]),
    "gamut_hip_qoix_plane_row_capacity": (_i, []),
    "gamut_hip_qoix_last_plane_kernel_ms": (_f, []),
    "gamut_hip_qoix_encode_bound": (_i64, [C.POINTER(QoixDesc)]),
    "gamut_hip_qoix_encode_batch_device": (_i, [C.POINTER(_vp), C.POINTER(_i64), C.POINTER(QoixDesc), _i, C.POINTER(_i64), _vp,
                                            C.POINTER(_i64), _pi, _vp]),
    "gamut_hip_qoix_write_to_mem": (_vp, [_vp, _i, C.POINTER(QoixDesc), _pi]),
    "gamut_hip_qoix_encode_window": (_i, []),
    "gamut_hip_qoix_plane_encode_segment": (_i, []),
    "gamut_hip_lz4_compress_bound": (_i, [_i]),
    "gamut_hip_lz4_compress_batch_device": (_i, [C.POINTER(_vp), C.POINTER(C.c_int32), _i, C.POINTER(_i64), _vp, C.POINTER(_i64), _pi, _vp]),
    "gamut_hip_qoix_last_encode_kernel_ms": (_f, []),
    "gamut_hip_qoix_last_encode_stage_ms": (_f, [_i]),
    "gamut_hip_qoix_last_plane_encode_stage_ms": (_f, [_i]),
    "gamut_hip_sqz_read_header": (_i, [_vp, _sz, C.POINTER(SqzInfo)]),
    "gamut_hip_sqz_decode_coeffs": (_i, [_vp, _sz, _vp, _sz, C.POINTER(SqzInfo)]),
    "gamut_hip_sqz_reconstruct_batch_device": (_i, [_vp, C.POINTER(SqzDesc), _i, C.POINTER(_i64), _vp, _pi, _vp]),
    "gamut_hip_sqz_decode_batch_device": (_i, [C.POINTER(_vp), C.POINTER(_sz), _i, C.POINTER(_i64), _vp, C.POINTER(SqzInfo), _pi, _vp]),
    "gamut_hip_sqz_linear_to_srgb_table": (_vp, []),
    "gamut_hip_sqz_last_decode_stage_ms": (_f, [_i]),
    "gamut_hip_sqz_budget_from_flags": (_i64, [_i, _i, _i]),
    "gamut_hip_sqz_analyze_batch_device": (_i, [C.POINTER(_vp), C.POINTER(_i64), C.POINTER(SqzEncodeDesc), _i, _vp, C.POINTER(_i64), _pi, _vp]),
    "gamut_hip_sqz_dwt_batch_device": (_i, [_vp, C.POINTER(SqzEncodeDesc), _i, _vp, C.POINTER(_i64), _pi, _vp]),
    "gamut_hip_sqz_encode_coeffs": (_i, [_vp, C.POINTER(SqzEncodeDesc), _vp, C.POINTER(_i64)]),
    "gamut_hip_sqz_encode_batch_device": (_i, [C.POINTER(_vp), C.POINTER(_i64), C.POINTER(SqzEncodeDesc), _i, C.POINTER(_i64), _vp,
                                           C.POINTER(_i64), _pi, _vp]),
    "gamut_hip_sqz_write_to_mem": (_vp, [_vp, _i, C.POINTER(SqzEncodeDesc), _pi]),
    "gamut_hip_sqz_last_encode_stage_ms": (_f, [_i]),
    "gamut_hip_sqz_write_batch_device": (_i, [_vp, C.POINTER(_i64), C.POINTER(SqzEncodeDesc), _i, C.POINTER(_i64), _vp, C.POINTER(_i64), _pi, _vp]),
    "gamut_hip_sqz_encode_batch_to_device": (_i, [C.POINTER(_vp), C.POINTER(_i64), C.POINTER(SqzEncodeDesc), _i, C.POINTER(_i64), _vp,
                                              C.POINTER(_i64), _pi, _vp]),
    "gamut_hip_sqz_scan_order": (_i, [_i, _i, _i, _vp]),
    "gamut_hip_sqz_write_chunk": (_i, []),
    "gamut_hip_sqz_last_write_stage_ms": (_f, [_i]),
    "gamut_hip_sqz_set_writer": (_i, [_i]),
    "gamut_hip_sqz_read_batch_device": (_i, [C.POINTER(_vp), C.POINTER(_sz), _i, _vp, C.POINTER(_i64), C.POINTER(SqzInfo), _pi, _vp]),
    "gamut_hip_sqz_set_reader": (_i, [_i]),
    "gamut_hip_sqz_read_window": (_i, []),
    "gamut_hip_sqz_set_read_chunk": (_i64, [_i64]),
    "gamut_hip_sqz_last_read_stage_ms": (_f, [_i]),
    "gamut_hip_flip_device": (_i, [_i, _vp, _i64, _i64, _i, _i, _i, _i, _vp]),
    "gamut_hip_flip": (_i, [_i, _vp, _i, _i, _i, _i]),
    "gamut_hip_jpeg_read_header": (_i, [_vp, _sz, C.POINTER(JpegFrame)]),
    "gamut_hip_jpeg_scan_layout": (_i, [_vp, _sz, C.POINTER(JpegFrame), C.POINTER(C.c_int32), C.POINTER(C.c_uint64)]),
    "gamut_hip_jpeg_entropy_decode_device": (_i, [C.POINTER(_vp), C.POINTER(_sz), _i, C.POINTER(_i64), C.POINTER(_i64), _vp, _vp, _vp,
                                              C.POINTER(JpegFrame), C.POINTER(_i), _vp]),
    "gamut_hip_jpeg_decode_batch_device": (_i, [C.POINTER(_vp), C.POINTER(_sz), _i, _i, C.POINTER(_i64), _vp, C.POINTER(JpegFrame), C.POINTER(_i), _vp, _vp]),
    "gamut_hip_jpeg_decode_coeffs_batch": (_i, [C.POINTER(_vp), C.POINTER(_sz), _i, C.POINTER(JpegFrame), C.POINTER(_i), _i]),
    "gamut_hip_jpeg_frame_free": (None, [C.POINTER(JpegFrame)]),
    "gamut_hip_decompress_jpeg_image_from_memory": (_vp, [_vp, _sz, _pi, _pi, _pi, _pf, _pf, _i]),
    "gamut_hip_png_defilter_device": (_i, [C.POINTER(PngDesc), _i, _vp, _vp]),
    "gamut_hip_png_defilter_batch_device": (_i, [_vp, _i64, _u32, _vp, _i64, _u32, _u32, _i, _i, _i, _i, _i, _vp, _vp]),
    "gamut_hip_stbi_load_from_memory": (_vp, [_vp, _sz, _pi, _pi, _pi, _i, _pf, _pf, _pf]),
    "gamut_hip_stbi_load_16_from_memory": (_vp, [_vp, _sz, _pi, _pi, _pi, _i, _pf, _pf, _pf]),
    "gamut_hip_png_is16": (_i, [_vp, _sz]),
    "gamut_hip_decompress_jpeg_image_from_stream": (_vp, [_vp, _vp, _pi, _pi, _pi, _pf, _pf, _i]),
    "gamut_hip_stbi_load_from_callbacks": (_vp, [_vp, _vp, _pi, _pi, _pi, _i, _pf, _pf, _pf]),
    "gamut_hip_stbi_load_16_from_callbacks": (_vp, [_vp, _vp, _pi, _pi, _pi, _i, _pf, _pf, _pf]),
    "gamut_hip_stbi_png_is16_from_callbacks": (_i, [_vp, _vp]),
    "gamut_hip_inflate_batch_device": (_i, [_vp, _i, _vp, _vp, _vp]),
    "gamut_hip_inflate_batch_device_sliced": (_i, [_vp, _i, _vp, _vp, C.c_uint32, _vp]),
    "gamut_hip_identify_format": (_i, [_vp, _sz]),
    "gamut_hip_decode_batch_device": (_i, [C.POINTER(_vp), C.POINTER(_sz), _i, _i, C.POINTER(_i64), _vp, C.POINTER(ImageInfo), C.POINTER(_i), _vp]),
    "gamut_hip_shard_owner": (_i, [_i64, _i]),
    "gamut_hip_shard_count": (_i64, [_i, _i, _i64]),
    "gamut_hip_shard_local_index": (_i64, [_i64, _i]),
    "gamut_hip_shard_global_index": (_i64, [_i64, _i, _i]),
    "gamut_hip_host_threads": (_i, []),
    "gamut_hip_comm_get_unique_id": (_i, [_vp]),
    "gamut_hip_comm_init": (_i, [C.POINTER(_vp), _i, _i, _vp]),
    "gamut_hip_comm_destroy": (None, [_vp]),
    "gamut_hip_comm_rank": (_i, [_vp]),
    "gamut_hip_comm_world": (_i, [_vp]),
    "gamut_hip_gather_outputs_device": (_i, [_vp, _vp, _i64, _i64, _i64, _vp, _i64, _i, _vp]),
}

JPEG_STREAM_READ_FUNC = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_ubyte), C.c_void_p)      # jpegload.d:70
JPEG_WRITE_FUNC = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_int)                                     # stb_image_write.d stbi_write_func


class StbiIoCallbacks(C.Structure):                                                                       # stbdec.d:408-419
    _fields_ = [("read", C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_char), C.c_int)),
                ("skip", C.CFUNCTYPE(None, C.c_void_p, C.c_int)),
                ("eof", C.CFUNCTYPE(C.c_int, C.c_void_p))]

_lib = None


def lib():
    """Load libgamut_hip.so (raises if it has not been built: no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} not found: build it with `make -C gamut_amd/csrc` "
                              f"(or __graft_entry__.build()); gamut_amd has no CPU fallback")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)          # AttributeError if the library does not export it
            fn.restype, fn.argtypes = res, args
        # wake the HIP runtime the library is linked against NOW: a process that loads it, then lets PyTorch (which brings
        # its own copy of the runtime) find the GPU first, was seen to get "no device" from this one afterwards
        L.gamut_hip_device_count()
        _lib = L
    return _lib


def last_error():
    return lib().gamut_hip_last_error().decode("utf-8", "replace")


def check(status):
    if status != OK:
        raise GamutHipError(status, last_error())
