"""ctypes loader for libfpng_amd.so (the C ABI in include/fpng_amd.h).

torch is imported first ON PURPOSE: the PyTorch-ROCm wheel bundles its own libamdhip64.so.7; loading
it first makes our library (DT_NEEDED libamdhip64.so.7) bind to the same HIP runtime instance
instead of pulling in a second one from /opt/rocm.
"""
import ctypes as C
import os

import torch  # noqa: F401  (must precede the CDLL below, see module docstring)

_HERE = os.path.dirname(os.path.abspath(__file__))
# FPNG_AMD_LIB: developer override for A/B-timing two builds on the same GPU box
LIB_PATH = os.environ.get("FPNG_AMD_LIB") or os.path.join(_HERE, "lib", "libfpng_amd.so")

NUM_PHASES = 8


class Image(C.Structure):
    _fields_ = [("d_pixels", C.c_void_p), ("w", C.c_uint32), ("h", C.c_uint32), ("num_chans", C.c_uint32),
                ("d_out", C.c_void_p), ("out_cap", C.c_size_t)]


class ImageEx(C.Structure):
    _fields_ = [("d_pixels", C.c_void_p), ("row_pitch", C.c_int64), ("w", C.c_uint32), ("h", C.c_uint32), ("format", C.c_uint32),
                ("d_out", C.c_void_p), ("out_cap", C.c_size_t)]


class ImagePlanar(C.Structure):  # fpng_amd_image_planar: 56 bytes, no padding
    _fields_ = [("d_pixels", C.c_void_p), ("row_pitch", C.c_int64), ("plane_pitch", C.c_int64), ("w", C.c_uint32), ("h", C.c_uint32),
                ("num_chans", C.c_uint32), ("reserved", C.c_uint32), ("d_out", C.c_void_p), ("out_cap", C.c_size_t)]


class Result(C.Structure):
    _fields_ = [("png_size", C.c_uint64), ("mode", C.c_uint32), ("status", C.c_uint32)]


class HostImage(C.Structure):
    _fields_ = [("pixels", C.c_void_p), ("w", C.c_uint32), ("h", C.c_uint32), ("num_chans", C.c_uint32), ("reserved", C.c_uint32),
                ("out", C.c_void_p), ("out_cap", C.c_size_t), ("out_size", C.POINTER(C.c_size_t)), ("path", C.c_char_p)]


class Band(C.Structure):
    _fields_ = [("d_rows", C.c_void_p), ("d_row_above", C.c_void_p), ("w", C.c_uint32), ("num_chans", C.c_uint32),
                ("y0", C.c_uint32), ("y1", C.c_uint32), ("h_total", C.c_uint32), ("reserved", C.c_uint32)]


class BandStats(C.Structure):
    _fields_ = [("token_bits", C.c_uint64), ("adler_s1", C.c_uint32), ("adler_s2", C.c_uint32),
                ("adler_len", C.c_uint64), ("last_unit_bits", C.c_uint32), ("first_token_bit", C.c_uint32),
                ("eob_bits", C.c_uint32), ("reserved", C.c_uint32)]


class PngIn(C.Structure):
    _fields_ = [("data", C.c_void_p), ("size", C.c_uint32), ("reserved", C.c_uint32), ("d_pixels", C.c_void_p), ("pixels_cap", C.c_size_t)]


class PngExIn(C.Structure):  # fpng_amd_png_ex: 40 bytes, no padding
    _fields_ = [("data", C.c_void_p), ("size", C.c_uint32), ("format", C.c_uint32), ("d_pixels", C.c_void_p), ("row_pitch", C.c_int64),
                ("pixels_cap", C.c_size_t)]


class PngPlanarIn(C.Structure):  # fpng_amd_png_planar: 48 bytes, no padding
    _fields_ = [("data", C.c_void_p), ("size", C.c_uint32), ("num_chans", C.c_uint32), ("d_pixels", C.c_void_p), ("row_pitch", C.c_int64),
                ("plane_pitch", C.c_int64), ("pixels_cap", C.c_size_t)]


class FloatFormat(C.Structure):  # fpng_amd_float_format: 40 bytes
    _fields_ = [("dtype", C.c_uint32), ("reserved", C.c_uint32), ("scale", C.c_float * 4), ("bias", C.c_float * 4)]


F32, F16, BF16 = 0, 1, 2  # FPNG_AMD_F32 / _F16 / _BF16


class Crop(C.Structure):  # fpng_amd_crop: 16 bytes, in pixels of the file, top-down
    _fields_ = [("x", C.c_uint32), ("y", C.c_uint32), ("w", C.c_uint32), ("h", C.c_uint32)]


DECODE_CROP_OUTSIDE = 67  # FPNG_AMD_DECODE_CROP_OUTSIDE: a file's status when its crop leaves the image


class Resize(C.Structure):  # fpng_amd_resize: 16 bytes, the output size of a file's crop
    _fields_ = [("out_w", C.c_uint32), ("out_h", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class ResizeView(C.Structure):  # fpng_amd_resize_view: 32 bytes, a window of a file's crop resized to full_w x full_h
    _fields_ = [("full_w", C.c_uint32), ("full_h", C.c_uint32), ("x", C.c_uint32), ("y", C.c_uint32), ("w", C.c_uint32), ("h", C.c_uint32),
                ("flags", C.c_uint32), ("filter", C.c_uint32)]


class ViewDest(C.Structure):  # fpng_amd_view_dest: 32 bytes, the destination of ONE view of fpng_amd_decode_batch(_device)_planar_views
    _fields_ = [("d_pixels", C.c_void_p), ("row_pitch", C.c_int64), ("plane_pitch", C.c_int64), ("pixels_cap", C.c_size_t)]


class ViewDestHwc(C.Structure):  # fpng_amd_view_dest_hwc: 32 bytes, the channels-last destination of ONE view of fpng_amd_decode_batch(_device)_hwc_views
    _fields_ = [("d_pixels", C.c_void_p), ("row_pitch", C.c_int64), ("pixel_elems", C.c_uint32), ("flags", C.c_uint32), ("pixels_cap", C.c_size_t)]


class ViewColor(C.Structure):  # fpng_amd_view_color: 64 bytes, the colour matrix of ONE view of the _views_color calls
    _fields_ = [("m", (C.c_float * 4) * 3), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class ViewPost(C.Structure):  # fpng_amd_view_post: 32 bytes, the post-processing record of ONE view of the _views_post calls
    _fields_ = [("flags", C.c_uint32), ("blur_radius", C.c_uint32), ("blur_sigma", C.c_double), ("solarize_threshold", C.c_uint32), ("posterize_bits", C.c_uint32),
                ("reserved", C.c_uint32 * 2)]


class ViewWarp(C.Structure):  # fpng_amd_view_warp: 64 bytes, the affine warp record of ONE view of the _views_warp calls
    _fields_ = [("flags", C.c_uint32), ("reserved0", C.c_uint32), ("a", C.c_double * 6), ("fill", C.c_uint8 * 4), ("reserved1", C.c_uint32)]


class ViewTone(C.Structure):  # fpng_amd_view_tone: 16 bytes, the tone record of ONE view of the _views_tone calls
    _fields_ = [("op", C.c_uint32), ("factor", C.c_float), ("reserved", C.c_uint32 * 2)]


class ViewEnhance(C.Structure):  # fpng_amd_view_enhance: 16 bytes, the enhance record of ONE view of the _views_enhance calls
    _fields_ = [("op", C.c_uint32), ("factor", C.c_float), ("reserved", C.c_uint32 * 2)]


class ViewAlpha(C.Structure):  # fpng_amd_view_alpha: 16 bytes, the alpha record of ONE view of the _views_alpha calls
    _fields_ = [("op", C.c_uint32), ("background", C.c_uint8 * 4), ("reserved", C.c_uint32 * 2)]


class ViewResample(C.Structure):  # fpng_amd_view_resample: 16 bytes, the RESAMPLE record of ONE view of the _views_resample calls
    _fields_ = [("filter", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 2)]


POST_BLUR, POST_SOLARIZE, POST_POSTERIZE = 1, 2, 4  # FPNG_AMD_POST_*
TONE_AUTOCONTRAST, TONE_EQUALIZE, TONE_CONTRAST = 1, 2, 3  # FPNG_AMD_TONE_*
ENHANCE_BRIGHTNESS, ENHANCE_COLOR, ENHANCE_SHARPNESS = 1, 2, 3  # FPNG_AMD_ENHANCE_*
ALPHA_COMPOSITE, ALPHA_PREMULTIPLIED = 1, 2  # FPNG_AMD_ALPHA_*
RESAMPLE_NEAREST, RESAMPLE_BOX, RESAMPLE_HAMMING, RESAMPLE_LANCZOS = 1, 2, 3, 4  # FPNG_AMD_RESAMPLE_*
WARP_AFFINE, WARP_BILINEAR = 1, 2  # FPNG_AMD_WARP_*
BLUR_MAX_RADIUS = 16  # FPNG_AMD_BLUR_MAX_RADIUS
HWC_REVERSED = 1  # FPNG_AMD_HWC_REVERSED
FILTER_BILINEAR, FILTER_BICUBIC = 0, 1  # FPNG_AMD_FILTER_*
RESIZE_MIRROR = 1  # FPNG_AMD_RESIZE_MIRROR
RESIZE_MAX_TAPS = 65  # weights per output sample of fpng_amd_resize_weights


class Pack(C.Structure):  # fpng_amd_pack: 40 bytes
    _fields_ = [("d_arena", C.c_void_p), ("arena_cap", C.c_uint64), ("align", C.c_uint32), ("lead", C.c_uint32), ("d_table", C.c_void_p),
                ("reserved", C.c_uint64)]


class PackedResult(C.Structure):  # fpng_amd_packed_result: 24 bytes
    _fields_ = [("offset", C.c_uint64), ("png_size", C.c_uint64), ("mode", C.c_uint32), ("status", C.c_uint32)]


DESC_IMAGE, DESC_EX, DESC_PLANAR, DESC_PLANAR_FLOAT = 0, 1, 2, 3  # FPNG_AMD_DESC_*


class Rendition(C.Structure):  # fpng_amd_rendition: 56 bytes, no padding
    _fields_ = [("image", C.c_uint32), ("filter", C.c_uint32), ("box_x", C.c_uint32), ("box_y", C.c_uint32), ("box_w", C.c_uint32), ("box_h", C.c_uint32),
                ("w", C.c_uint32), ("h", C.c_uint32), ("alpha_op", C.c_uint32), ("reserved", C.c_uint32), ("d_out", C.c_void_p), ("out_cap", C.c_size_t)]


# FPNG_AMD_RENDITION_*: one numbering for the six filters
RENDITION_FILTERS = {"bilinear": 0, "bicubic": 1, "nearest": 2, "box": 3, "hamming": 4, "lanczos": 5}


class YuvFrame(C.Structure):  # fpng_amd_yuv_frame: 56 bytes, no padding
    _fields_ = [("d_luma", C.c_void_p), ("row_pitch", C.c_int64), ("chroma_offset", C.c_int64), ("w", C.c_uint32), ("h", C.c_uint32),
                ("reserved", C.c_uint64), ("d_out", C.c_void_p), ("out_cap", C.c_size_t)]


class YuvFormat(C.Structure):  # fpng_amd_yuv_format: 56 bytes
    _fields_ = [("surface", C.c_uint32), ("reserved", C.c_uint32), ("m", (C.c_float * 4) * 3)]


class YuvDest(C.Structure):  # fpng_amd_yuv_dest: 40 bytes
    _fields_ = [("d_luma", C.c_void_p), ("row_pitch", C.c_int64), ("chroma_offset", C.c_int64), ("surface_cap", C.c_size_t), ("reserved", C.c_uint64)]


class YuvStoreFormat(C.Structure):  # fpng_amd_yuv_store_format: 56 bytes
    _fields_ = [("surface", C.c_uint32), ("depth", C.c_uint32), ("m", (C.c_float * 4) * 3)]


YUV_SURFACES = {"nv12": 0, "p016": 1, "yuv444": 2, "yuv444_16": 3}  # FPNG_AMD_YUV_* (p016 serves P010 / P012)
YUV_STANDARDS = {"bt601": 0, "bt709": 1, "bt2020": 2}  # FPNG_AMD_YUV_BT*


class DecodeResult(C.Structure):
    _fields_ = [("w", C.c_uint32), ("h", C.c_uint32), ("channels_in_file", C.c_uint32), ("status", C.c_int32)]


# fpng_amd_decode_batch(_device)_png: the general decode tier for ordinary PNG files
DECODE_UNSUPPORTED_PNG = 67  # FPNG_AMD_DECODE_UNSUPPORTED_PNG: a valid PNG the tier does not decode (other bit depths, interlace, unknown critical chunks)
PNG_GENERAL_ONLY = 1  # FPNG_AMD_PNG_GENERAL_ONLY: flags -- every file through the general tier, fpng-written ones too


class BandPlan(C.Structure):
    _fields_ = [("end_bit", C.c_uint64), ("zlib_size", C.c_uint64), ("adler", C.c_uint32), ("stored", C.c_uint32)]


RESERVE_FN = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_size_t)


class Transport(C.Structure):
    """fpng_amd_transport: the exchange functions fpng_amd_encode_image_sharded() calls (all on the encoder's stream)."""
    _fields_ = [("ctx", C.c_void_p), ("rank", C.c_int), ("world", C.c_int),
                ("all_gather", C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)),
                ("all_reduce_sum_u32", C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)),
                ("group_begin", C.CFUNCTYPE(C.c_int, C.c_void_p)),
                ("send", C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p)),
                ("recv", C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p)),
                ("group_end", C.CFUNCTYPE(C.c_int, C.c_void_p))]

# every symbol include/fpng_amd.h declares: (restype, argtypes)
_u32, _u64, _sz, _vp, _int = C.c_uint32, C.c_uint64, C.c_size_t, C.c_void_p, C.c_int


class RuntimeInfo(C.Structure):
    """fpng_amd_runtime (include/fpng_amd.h)"""
    _fields_ = [("hw_queues", _u32), ("hw_queue_source", _u32), ("lanes", _u32), ("reserved", _u32 * 5)]


SIGNATURES = {
    "fpng_amd_init": (_int, [_int]),
    "fpng_amd_device_available": (_int, []),
    "fpng_amd_device_count": (_int, []),
    "fpng_amd_last_error": (C.c_char_p, []),
    "fpng_amd_abi_version": (_int, []),
    "fpng_amd_crc32": (_u32, [_vp, _sz, _u32]),
    "fpng_amd_adler32": (_u32, [_vp, _sz, _u32]),
    "fpng_amd_crc32_combine": (_u32, [_u32, _u32, _u64]),
    "fpng_amd_adler32_combine": (_u32, [_u32, _u32, _u64]),
    "fpng_amd_max_encoded_size": (_sz, [_u32, _u32, _u32]),
    "fpng_amd_encoder_create": (_int, [C.POINTER(_vp), _int, _vp]),
    "fpng_amd_encoder_create_on_stream": (_int, [C.POINTER(_vp), _int, _vp]),
    "fpng_amd_encoder_set_stream": (_int, [_vp, _vp]),
    "fpng_amd_encoder_destroy": (None, [_vp]),
    "fpng_amd_encoder_stream": (_vp, [_vp]),
    "fpng_amd_encoder_join": (_int, [_vp]),
    "fpng_amd_encoder_phase_names": (C.c_char_p, [_vp]),
    "fpng_amd_encode_batch_async": (_int, [_vp, C.POINTER(Image), _u32, _u32]),
    "fpng_amd_encode_finish": (_int, [_vp, C.POINTER(Result), _u32]),
    "fpng_amd_encode_submit": (_int, [_vp, C.POINTER(Image), _u32, _u32, C.POINTER(_u64)]),
    "fpng_amd_encode_submit_ex": (_int, [_vp, C.POINTER(ImageEx), _u32, _u32, C.POINTER(_u64)]),
    "fpng_amd_encode_submit_planar": (_int, [_vp, C.POINTER(ImagePlanar), _u32, _u32, C.POINTER(_u64)]),
    "fpng_amd_encode_submit_planar_float": (_int, [_vp, C.POINTER(ImagePlanar), _u32, C.POINTER(FloatFormat), _u32, C.POINTER(_u64)]),
    "fpng_amd_quantize_float": (_int, [_vp, _u32, C.c_float, C.c_float, _vp, _sz]),
    "fpng_amd_encode_submit_packed": (_int, [_vp, _u32, _vp, _u32, C.POINTER(FloatFormat), _u32, C.POINTER(Pack), C.POINTER(_u64)]),
    "fpng_amd_encode_wait_packed": (_int, [_vp, _u64, C.POINTER(PackedResult), _u32, C.POINTER(_u64)]),
    "fpng_amd_pack_place": (_int, [C.POINTER(_u64), C.POINTER(_u32), _u32, _u32, _u32, _u64, C.POINTER(_u64), C.POINTER(_u32), C.POINTER(_u64)]),
    "fpng_amd_pack_capacity": (_sz, [C.POINTER(_u32), C.POINTER(_u32), C.POINTER(_u32), _u32, _u32, _u32]),
    "fpng_amd_encode_submit_renditions": (_int, [_vp, _u32, _vp, _u32, C.POINTER(FloatFormat), C.POINTER(Rendition), _u32, _u32, C.POINTER(Pack), C.POINTER(_u64)]),
    "fpng_amd_renditions_plan": (_int, [_u32, _vp, _u32, C.POINTER(FloatFormat), C.POINTER(Rendition), _u32, _int, C.POINTER(_u64), C.POINTER(_u64)]),
    "fpng_amd_rendition_pixels": (_int, [_u32, _vp, _u32, C.POINTER(FloatFormat), C.POINTER(Rendition), _vp, _sz]),
    "fpng_amd_encode_submit_yuv": (_int, [_vp, C.POINTER(YuvFrame), _u32, C.POINTER(YuvFormat), C.POINTER(Rendition), _u32, _u32, C.POINTER(Pack), C.POINTER(_u64)]),
    "fpng_amd_yuv_matrix": (_int, [_u32, _int, C.POINTER(C.c_float)]),
    "fpng_amd_yuv_pixels": (_int, [C.POINTER(YuvFrame), _u32, C.POINTER(YuvFormat), _u32, C.POINTER(Rendition), _vp, _sz]),
    "fpng_amd_encode_wait": (_int, [_vp, _u64, C.POINTER(Result), _u32]),
    "fpng_amd_encode_query": (_int, [_vp, _u64]),
    "fpng_amd_encode_host": (_int, [_vp, _vp, _u32, _u32, _u32, _u32, _vp, _sz, C.POINTER(_sz)]),
    "fpng_amd_encode_host_batch": (_int, [_vp, C.POINTER(HostImage), _u32, _u32, _int]),
    "fpng_amd_band_hist": (_int, [_vp, C.POINTER(Band), _vp]),
    "fpng_amd_band_encode": (_int, [_vp, C.POINTER(Band), _u32, _vp, C.POINTER(BandStats)]),
    "fpng_amd_band_place": (_int, [_vp, C.POINTER(Band), _u64, _u64, _vp, _sz, C.POINTER(_u64), C.POINTER(_sz)]),
    "fpng_amd_1pass_layout": (_int, [_u32, C.POINTER(_u32), C.POINTER(_u32), C.POINTER(_u32)]),
    "fpng_amd_wrap_png": (_int, [_vp, _vp, _sz, _u32, _u32, _u32, _u32, C.POINTER(_sz)]),
    "fpng_amd_wrap_png_crc": (_int, [_vp, _vp, _sz, _u32, _u32, _u32, _u32, _vp, _u32, C.POINTER(_sz)]),
    "fpng_amd_band_crc_partials": (_int, [_vp, _vp, _u32, C.POINTER(_u32)]),
    "fpng_amd_band_crc": (_int, [_vp, C.POINTER(_u32), C.POINTER(_u64)]),
    "fpng_amd_plan_bands": (_int, [C.POINTER(BandStats), _u32, _u32, _u32, _u32, _u32, C.POINTER(_u64), C.POINTER(BandPlan)]),
    "fpng_amd_band_window": (_int, [_int, _int, _u64, _u64, _u32, C.POINTER(_u64), C.POINTER(_sz), C.POINTER(_u32)]),
    "fpng_amd_idat_crc_from_bands": (_u32, [C.POINTER(_u32), C.POINTER(_u64), _u32, _u64, _u32]),
    "fpng_amd_png_head": (_int, [_u32, _u32, _u32, _u64, _vp]),
    "fpng_amd_png_tail": (None, [_u32, _u32, _vp]),
    "fpng_amd_encode_host_to": (_int, [_vp, _vp, _u32, _u32, _u32, _u32, RESERVE_FN, _vp, C.POINTER(_sz)]),
    "fpng_amd_rccl_unique_id": (_int, [_vp]),
    "fpng_amd_rccl_transport_create": (_int, [C.POINTER(C.POINTER(Transport)), _vp, _int, _int, _int]),
    "fpng_amd_rccl_transport_destroy": (None, [C.POINTER(Transport)]),
    "fpng_amd_encode_image_sharded": (_int, [_vp, C.POINTER(Transport), C.POINTER(Band), _u32, _int, _vp, _sz, C.POINTER(_sz)]),
    "fpng_amd_sharded_last_report": (_int, [_vp, _vp]),
    "fpng_amd_encoder_last_host_bands": (_int, [_vp]),
    "fpng_amd_pin_host_memory": (_int, [_vp, _sz]),
    "fpng_amd_unpin_host_memory": (_int, [_vp]),
    "fpng_amd_node_create": (_int, [C.POINTER(_vp), C.POINTER(_int), _u32]),
    "fpng_amd_node_destroy": (None, [_vp]),
    "fpng_amd_node_size": (_u32, [_vp]),
    "fpng_amd_node_encode_host_batch": (_int, [_vp, C.POINTER(HostImage), _u32, _u32, _int]),
    "fpng_amd_node_encode_host_image": (_int, [_vp, _vp, _u32, _u32, _u32, _u32, RESERVE_FN, _vp, C.POINTER(_sz)]),
    "fpng_amd_decode_batch": (_int, [_vp, C.POINTER(PngIn), _u32, _u32, C.POINTER(DecodeResult)]),
    "fpng_amd_decode_batch_device": (_int, [_vp, C.POINTER(PngIn), _u32, _u32, C.POINTER(DecodeResult)]),
    "fpng_amd_decode_batch_png": (_int, [_vp, C.POINTER(PngIn), _u32, _u32, _u32, C.POINTER(DecodeResult)]),
    "fpng_amd_decode_batch_device_png": (_int, [_vp, C.POINTER(PngIn), _u32, _u32, _u32, C.POINTER(DecodeResult)]),
    "fpng_amd_decode_png_last_kernel_ms": (_int, [_vp, C.POINTER(C.c_float * 2)]),
    "fpng_amd_decode_batch_ex": (_int, [_vp, C.POINTER(PngExIn), _u32, C.POINTER(DecodeResult)]),
    "fpng_amd_decode_batch_device_ex": (_int, [_vp, C.POINTER(PngExIn), _u32, C.POINTER(DecodeResult)]),
    "fpng_amd_decode_batch_planar": (_int, [_vp, C.POINTER(PngPlanarIn), _u32, C.POINTER(DecodeResult)]),
    "fpng_amd_decode_batch_device_planar": (_int, [_vp, C.POINTER(PngPlanarIn), _u32, C.POINTER(DecodeResult)]),
    "fpng_amd_decode_batch_planar_float": (_int, [_vp, C.POINTER(PngPlanarIn), _u32, C.POINTER(FloatFormat), C.POINTER(DecodeResult)]),
    "fpng_amd_decode_batch_device_planar_float": (_int, [_vp, C.POINTER(PngPlanarIn), _u32, C.POINTER(FloatFormat), C.POINTER(DecodeResult)]),
    "fpng_amd_decode_batch_planar_crop": (_int, [_vp, C.POINTER(PngPlanarIn), C.POINTER(Crop), _u32, C.POINTER(FloatFormat), C.POINTER(DecodeResult)]),
    "fpng_amd_decode_batch_device_planar_crop": (_int, [_vp, C.POINTER(PngPlanarIn), C.POINTER(Crop), _u32, C.POINTER(FloatFormat), C.POINTER(DecodeResult)]),
    "fpng_amd_decode_batch_planar_resize": (_int, [_vp, C.POINTER(PngPlanarIn), C.POINTER(Crop), C.POINTER(Resize), _u32, C.POINTER(FloatFormat), C.POINTER(DecodeResult)]),
    "fpng_amd_decode_batch_device_planar_resize": (_int, [_vp, C.POINTER(PngPlanarIn), C.POINTER(Crop), C.POINTER(Resize), _u32, C.POINTER(FloatFormat), C.POINTER(DecodeResult)]),
    "fpng_amd_resize_weights": (_int, [_u32, _u32, C.POINTER(_u32), C.POINTER(_u32), C.POINTER(C.c_int32)]),
    "fpng_amd_decode_batch_planar_resize_view": (_int, [_vp, C.POINTER(PngPlanarIn), C.POINTER(Crop), C.POINTER(ResizeView), _u32, C.POINTER(FloatFormat), C.POINTER(DecodeResult)]),
    "fpng_amd_decode_batch_device_planar_resize_view": (_int, [_vp, C.POINTER(PngPlanarIn), C.POINTER(Crop), C.POINTER(ResizeView), _u32, C.POINTER(FloatFormat), C.POINTER(DecodeResult)]),
    "fpng_amd_resize_weights_filter": (_int, [_u32, _u32, _u32, C.POINTER(_u32), C.POINTER(_u32), C.POINTER(C.c_int32)]),
    "fpng_amd_resize_view_source": (_int, [C.POINTER(Crop), C.POINTER(ResizeView), C.POINTER(Crop)]),
    "fpng_amd_view_warp_apply": (_int, [C.POINTER(ViewWarp), _u32, _u32, _u32, C.c_void_p, C.c_void_p, C.c_uint8]),
    "fpng_amd_view_tone_lut": (_int, [C.POINTER(ViewTone), C.c_void_p, C.c_void_p]),
    "fpng_amd_view_tone_apply": (_int, [C.POINTER(ViewTone), _u32, _u32, C.c_void_p, C.c_void_p]),
    "fpng_amd_view_enhance_apply": (_int, [C.POINTER(ViewEnhance), _u32, _u32, C.c_void_p, C.c_void_p]),
    "fpng_amd_resample_weights": (_int, [_u32, _u32, _u32, C.POINTER(_u32), C.POINTER(_u32), C.POINTER(C.c_int32)]),
    "fpng_amd_resample_view_source": (_int, [C.POINTER(Crop), C.POINTER(ResizeView), C.POINTER(ViewResample), C.POINTER(Crop)]),
    "fpng_amd_view_alpha_source": (_int, [C.POINTER(ViewAlpha), _u32, _u32, C.c_void_p, C.c_void_p]),
    "fpng_amd_view_alpha_result": (_int, [C.POINTER(ViewAlpha), _u32, _u32, C.c_void_p, C.c_void_p]),
    "fpng_amd_blur_weights": (_int, [_u32, C.c_double, C.POINTER(C.c_int32 * 17)]),
    "fpng_amd_view_post_apply": (_int, [C.POINTER(ViewPost), _u32, _u32, C.c_void_p, C.c_void_p]),
    "fpng_amd_color_apply": (None, [C.POINTER(ViewColor), C.POINTER(C.c_uint8 * 3), C.POINTER(C.c_float * 3)]),
    "fpng_amd_views_source": (_int, [C.POINTER(Crop), C.POINTER(ResizeView), _u32, C.POINTER(Crop)]),
    "fpng_amd_decode_crop_tiles": (_int, [_u32, _u32, C.POINTER(Crop), C.POINTER(_u32), C.POINTER(_u32), C.POINTER(_u32)]),
    "fpng_amd_encoder_set_decode_verify": (_int, [_vp, _u32]),
    "fpng_amd_encoder_decode_verify": (_u32, [_vp]),
    "fpng_amd_decode_last_phase_ms": (_int, [_vp, C.POINTER(C.c_float * 4)]),
    "fpng_amd_decode_host": (_int, [_vp, _vp, _u32, _u32, RESERVE_FN, _vp, C.POINTER(DecodeResult)]),
    "fpng_amd_decode_plan": (_int, [_vp, _u32, C.POINTER(DecodeResult), C.POINTER(_u32), C.POINTER(_u32), C.POINTER(_u32), C.POINTER(C.c_uint64),
                             C.POINTER(C.c_uint64), C.POINTER(_u32 * 4160)]),
    "fpng_amd_train_tables": (_int, [_vp, C.POINTER(Image), _u32, _u32, _vp, _sz, C.POINTER(_sz), C.POINTER(_u32), C.POINTER(_u32), _vp, _vp]),
    "fpng_amd_synth_image": (_int, [_int, _u32, _u32, _u32, _u32, _vp]),
    "fpng_amd_encoder_set_profiling": (_int, [_vp, _int]),
    "fpng_amd_encoder_last_phase_ms": (_int, [_vp, C.POINTER(C.c_float * NUM_PHASES)]),
    "fpng_amd_debug_peek": (_int, [_vp, _int, C.POINTER(_u32), _u32]),
    "fpng_amd_runtime_info": (_int, [C.POINTER(RuntimeInfo)]),
    "fpng_amd_encoder_lanes": (_u32, [_vp]),
    "fpng_amd_release_cached_memory": (_int, []),
}

# The views calls: fpng_amd_decode_batch(_device)_{planar,hwc}_views<suffix>.  A stage's call takes the record arrays of every stage up
# to and including its own, in this order, between the destinations and the float format.
VIEW_STAGES = (("_color", ViewColor), ("_post", ViewPost), ("_warp", ViewWarp), ("_tone", ViewTone), ("_enhance", ViewEnhance), ("_alpha", ViewAlpha),
               ("_resample", ViewResample))
VIEW_LAYOUTS = (("planar", ViewDest), ("hwc", ViewDestHwc))


def views_symbol(layout, device_data, stages):
    """the name of the views call of `layout` ("planar" / "hwc") for files in device or host memory that takes the first `stages`
    record arrays of VIEW_STAGES"""
    return f"fpng_amd_decode_batch{'_device' if device_data else ''}_{layout}_views{VIEW_STAGES[stages - 1][0] if stages else ''}"


for _layout, _dest in VIEW_LAYOUTS:
    for _stages in range(len(VIEW_STAGES) + 1):
        for _device in (False, True):
            SIGNATURES[views_symbol(_layout, _device, _stages)] = (_int, [_vp, C.POINTER(PngPlanarIn), _u32, C.POINTER(_u32), C.POINTER(Crop), C.POINTER(ResizeView), C.POINTER(_dest)] +
                                                                  [C.POINTER(rec) for _, rec in VIEW_STAGES[:_stages]] + [C.POINTER(FloatFormat), C.POINTER(DecodeResult)])

# the YUV views call takes the plain views call's arrays with fpng_amd_yuv_dest records and its own format
for _device in (False, True):
    SIGNATURES[views_symbol("yuv", _device, 0)] = (_int, [_vp, C.POINTER(PngPlanarIn), _u32, C.POINTER(_u32), C.POINTER(Crop), C.POINTER(ResizeView), C.POINTER(YuvDest),
                                                          C.POINTER(YuvStoreFormat), C.POINTER(DecodeResult)])

# fpng_amd_decode_batch(_device)_png_views: views of ordinary PNG files, every family through one request record
DECODE_PNG_CROP_OUTSIDE = 68  # FPNG_AMD_DECODE_PNG_CROP_OUTSIDE: a file's status when a crop of it leaves the image (67 there: UNSUPPORTED_PNG)


class PngViews(C.Structure):  # fpng_amd_png_views: 112 bytes
    _fields_ = [("view_count", C.POINTER(_u32)), ("crops", C.POINTER(Crop)), ("views", C.POINTER(ResizeView)), ("dests", C.POINTER(ViewDest)), ("hwc", C.POINTER(ViewDestHwc)),
                ("fmt", C.POINTER(FloatFormat))] + [(name[1:] + "s", C.POINTER(rec)) for name, rec in VIEW_STAGES] + [("flags", _u32), ("reserved", _u32)]


def png_views_symbol(device_data):
    return f"fpng_amd_decode_batch{'_device' if device_data else ''}_png_views"


for _device in (False, True):
    SIGNATURES[png_views_symbol(_device)] = (_int, [_vp, C.POINTER(PngPlanarIn), _u32, C.POINTER(PngViews), C.POINTER(DecodeResult)])
SIGNATURES["fpng_amd_yuv_matrix_from_rgb"] =(_int, [_u32, _int, C.POINTER(C.c_float)])
SIGNATURES["fpng_amd_yuv_surface"] = (_int, [_vp, _u32, _u32, C.POINTER(YuvStoreFormat), C.POINTER(YuvDest)])

_lib = None


def load():
    """Load the library (built by `python -m fpng_amd.build` / __graft_entry__.build()).
    Fails loudly if it is missing: there is no Python or CPU fallback for the encode path."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} not found: build it with `python -m fpng_amd.build` "
                          "(fpng_amd has no CPU fallback)")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError here = ABI mismatch
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


class FpngAmdError(RuntimeError):
    def __init__(self, code, what):
        super().__init__(f"fpng_amd error {code}: {what}")
        self.code = code


def check(rc):
    if rc != 0:
        raise FpngAmdError(rc, load().fpng_amd_last_error().decode("utf-8", "replace"))
