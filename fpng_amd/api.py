"""Host-side mirror of the reference's `namespace fpng` encode interface (reference src/fpng.h:17-52)
on top of the C ABI, plus the device-resident batch / row-band entry points the MI355X path adds.

Names, argument meaning and error behaviour follow the reference:

    fpng_init()                                           src/fpng.h:17
    fpng_cpu_supports_sse41()  -> "is the accelerator usable"   src/fpng.h:23
    fpng_crc32(data, prev=0) / fpng_adler32(data, prev=1)        src/fpng.h:26-31
    fpng_encode_image_to_memory(image, w, h, num_chans, flags) -> (ok, bytes)   src/fpng.h:48
    fpng_encode_image_to_file(filename, image, w, h, num_chans, flags) -> ok    src/fpng.h:52

torch is only plumbing here (device memory + streams).  There is no CPU fallback: if the HIP library
or a GPU is missing, encode calls raise.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from ._lib import Band, BandStats, FpngAmdError, HostImage, Image, ImageEx, ImagePlanar, Result, check

FPNG_ENCODE_SLOWER = 1        # reference src/fpng.h:38
FPNG_FORCE_UNCOMPRESSED = 2   # reference src/fpng.h:41
FPNG_CRC32_INIT = 0           # reference src/fpng.h:26
FPNG_ADLER32_INIT = 1         # reference src/fpng.h:30

MODE_COMPRESSED, MODE_STORED = 0, 1
# fpng_amd_result.status / fpng_amd_packed_result.status
STATUS_STORED_TOO_LARGE, STATUS_ARENA_FULL = 1, 2

# Encoder.set_decode_verify (FPNG_AMD_VERIFY_* in include/fpng_amd.h) and the two statuses only a checked decode returns
VERIFY_CRC32, VERIFY_ADLER32 = 1, 2
DECODE_BAD_CRC32, DECODE_BAD_ADLER32 = 65, 66
# a file's status when its crop leaves the image (Encoder.decode_device_crop; FPNG_AMD_DECODE_CROP_OUTSIDE)
DECODE_CROP_OUTSIDE = _lib.DECODE_CROP_OUTSIDE
FPNG_AMD_DECODE_UNSUPPORTED_PNG = _lib.DECODE_UNSUPPORTED_PNG  # decode_device_png / decode_batch_png: a valid PNG the general tier does not decode
FPNG_AMD_PNG_GENERAL_ONLY = _lib.PNG_GENERAL_ONLY  # ... flags: every file through the general tier, fpng-written ones too
FPNG_AMD_DECODE_PNG_CROP_OUTSIDE = _lib.DECODE_PNG_CROP_OUTSIDE  # decode_device_png_views / decode_batch_png_views: a crop of the file leaves the image
# fpng_amd_resize.flags (Encoder.decode_device_resize: mirror=True sets it): the output's columns in reverse order
RESIZE_MIRROR = _lib.RESIZE_MIRROR
# fpng_amd_resize_view.filter (Encoder.decode_device_resize_view: filter="bilinear" / "bicubic")
FILTER_BILINEAR, FILTER_BICUBIC = _lib.FILTER_BILINEAR, _lib.FILTER_BICUBIC

# source formats of Encoder.submit_ex (FPNG_AMD_SRC_* in include/fpng_amd.h): name -> (value, source bytes per pixel, PNG channels)
SRC_FORMATS = {"RGB": (0, 3, 3), "BGR": (1, 3, 3), "RGBA": (2, 4, 4), "BGRA": (3, 4, 4), "ARGB": (4, 4, 4), "ABGR": (5, 4, 4),
               "RGBX": (6, 4, 3), "BGRX": (7, 4, 3), "XRGB": (8, 4, 3), "XBGR": (9, 4, 3)}
SRC_RGB, SRC_BGR, SRC_RGBA, SRC_BGRA, SRC_ARGB, SRC_ABGR, SRC_RGBX, SRC_BGRX, SRC_XRGB, SRC_XBGR = range(10)


def format_channels(fmt):
    """Channel count of the PNG a FPNG_AMD_SRC_* format is encoded to."""
    return [v[2] for v in SRC_FORMATS.values() if v[0] == fmt][0]


def _view_rows(t, who):
    """(h, w, c, pixel bytes) of a uint8 (h, w, c) tensor view whose channels are adjacent bytes, 3 or 4 of them in pixels of 3 or 4
    bytes, checked (source_layout / dest_layout)"""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 3:
        raise ValueError(f"{who}: a uint8 tensor shaped (h, w, c)")
    h, w, c = t.shape
    if c not in (3, 4) or h < 1 or w < 1:
        raise ValueError(f"{who}: {c} channels (3 or 4), {w} x {h}")
    if c > 1 and t.stride(2) != 1:
        raise ValueError(f"{who}: the channels of a pixel must be adjacent bytes (stride(2) == 1)")
    px = t.stride(1) if w > 1 else (4 if (t.stride(1) == 4 or c == 4) else 3)
    if px not in (3, 4) or px < c:
        raise ValueError(f"{who}: pixel stride {t.stride(1)} (3 or 4 bytes, at least the channels)")
    return h, w, c, px


def _row_pitch(t, ptr, h, w, px, bottom_up, who):
    """(base, signed row pitch) of the view's rows: 0 for a single row; bottom_up: the tensor's row 0 is the image's bottom row"""
    rp = t.stride(0)
    if h > 1 and (rp == 0 or rp < w * px):
        raise ValueError(f"{who}: row stride {rp} < w * {px} (rows overlap, or stride 0)")
    if h == 1:
        rp = 0  # (one row: no pitch)
    if bottom_up and h > 1:
        ptr, rp = ptr + (h - 1) * rp, -rp
    return ptr, rp


def source_layout(t, order="rgb", bottom_up=False):
    """(d_pixels, row_pitch, format) of a uint8 (h, w, c) tensor VIEW for Encoder.submit_ex, from its strides and data_ptr() alone
    (the device is not touched, so CPU tensors work too).

    order: the channel order of the view's c channels -- "rgb" / "bgr" for c = 3, "rgba" / "bgra" / "argb" / "abgr" for c = 4
    ("rgb" / "bgr" there mean alpha last).  stride(2) must be 1 and stride(1), the source pixel, 3 or 4 bytes.  A 3-channel view
    with 4-byte pixels ([..., :3] of RGBA) is an *X format; one whose first byte is the pixel's second byte ([..., 1:] of ARGB) an
    X*** format, its base moved back one byte.  bottom_up: the tensor's row 0 is the image's BOTTOM row (a GL readback): the file
    starts with the tensor's last row and the pitch is negative.  Rows that overlap, stride 0 and other dtypes are refused."""
    h, w, c, px = _view_rows(t, "source_layout")
    order = order.lower()
    if c == 4 and order in ("rgb", "bgr"):
        order += "a"
    if sorted(order) != sorted("rgba"[:c]):
        raise ValueError(f"source_layout: order {order!r} does not name the {c} channels")
    ptr = t.data_ptr()
    name = order.upper()
    if c == 3 and px == 4:
        # the ignored byte is the one the view leaves out: behind the channels on a dword boundary, else in front of them
        if ptr % 4 == 1:
            name, ptr = "X" + name, ptr - 1
        else:
            name += "X"
    ptr, rp = _row_pitch(t, ptr, h, w, px, bottom_up, "source_layout")
    return ptr, rp, SRC_FORMATS[name][0]


# destination bytes per pixel of an FPNG_AMD_SRC_* value when it names the pixel a decode writes (fpng_amd_decode_batch_ex)
def dest_bytes(fmt):
    return [v[1] for v in SRC_FORMATS.values() if v[0] == fmt][0]


def dest_layout(t, order="rgb", bottom_up=False):
    """(d_pixels, row_pitch, format) of a uint8 (h, w, c) tensor VIEW that a decode fills in place (Encoder.decode_device_ex /
    decode_batch_ex, fpng_amd_png_ex): the destination twin of source_layout(), from strides and data_ptr() alone.

    order: the view's channel order -- "rgb" / "bgr" for c = 3; for c = 4 "rgba" / "bgra" / "argb" / "abgr" ("rgb" / "bgr": alpha
    last) or, with an X byte the decoder sets to 0xFF, "rgbx" / "bgrx" / "xrgb" / "xbgr".  A 3-channel view of 4-byte pixels
    ([..., :3] of RGBA) is refused: the decoder writes whole pixels and would write the byte the view leaves out.  bottom_up: the
    tensor's row 0 is the image's BOTTOM row (the file's first row lands in the tensor's last).  Rows that overlap, stride 0 and
    other dtypes are refused."""
    h, w, c, px = _view_rows(t, "dest_layout")
    if px != c:
        raise ValueError(f"dest_layout: a {c}-channel view of {px}-byte pixels (the decoder would write the byte it leaves out)")
    order = order.lower()
    if c == 4 and order in ("rgb", "bgr"):
        order += "a"
    if sorted(order) not in ([sorted("rgb")] if c == 3 else [sorted("rgba"), sorted("rgbx")]):
        raise ValueError(f"dest_layout: order {order!r} does not name the {c} channels")
    ptr, rp = _row_pitch(t, t.data_ptr(), h, w, px, bottom_up, "dest_layout")
    return ptr, rp, SRC_FORMATS[order.upper()][0]


def _planar_layout(t, order, bottom_up, who, elem=None):
    """(d_pixels, row_pitch, plane_pitch) of a uint8 (c, h, w) tensor view: one plane of w-byte rows per channel.  elem: the view
    holds elements of that many bytes instead (dest_layout_float, which has checked the dtype): the same rules on its strides,
    which count elements, and the pitches returned in bytes"""
    if not isinstance(t, torch.Tensor) or (elem is None and t.dtype != torch.uint8) or t.dim() != 3:
        raise ValueError(f"{who}: a " + ("uint8" if elem is None else "float") + " tensor shaped (c, h, w)")
    c, h, w = t.shape
    if c not in (3, 4) or h < 1 or w < 1:
        raise ValueError(f"{who}: {c} planes (3 or 4), {w} x {h}")
    if w > 1 and t.stride(2) != 1:
        raise ValueError(f"{who}: the pixels of a row must be adjacent bytes (stride(2) == 1); stride(2) == {t.stride(2)} is an "
                         "interleaved view -- describe it as (h, w, c) with source_layout / dest_layout and use submit_ex / decode_device_ex, "
                         "or decode into it with decode_device_views_hwc")
    rp, pp = t.stride(1), t.stride(0)
    if h > 1 and rp < w:
        raise ValueError(f"{who}: row stride {rp} < w (rows overlap, or stride 0)")
    if h == 1:
        rp = 0  # (one row: no pitch)
    span = (h - 1) * rp + w  # bytes of a plane, from its first row's first byte
    if pp < span:
        raise ValueError(f"{who}: plane stride {pp} < (h - 1) * row stride + w = {span} (planes overlap, or stride 0)")
    order = order.lower()
    if c == 4 and order == "rgb":
        order = "rgba"
    if order not in (("rgb", "bgr") if c == 3 else ("rgba", "abgr")):
        raise ValueError(f"{who}: order {order!r} for {c} planes -- one base and one plane pitch can say "
                         + ("'rgb' or 'bgr'" if c == 3 else "'rgba' or 'abgr'") + " only")
    if elem is not None:
        rp, pp = rp * elem, pp * elem
    ptr = t.data_ptr()
    if order[0] != "r":  # the planes lie in reverse: start at the last one and walk back
        ptr, pp = ptr + (c - 1) * pp, -pp
    if bottom_up and h > 1:
        ptr, rp = ptr + (h - 1) * rp, -rp
    return ptr, rp, pp


def source_layout_planar(t, order="rgb", bottom_up=False):
    """(d_pixels, row_pitch, plane_pitch) of a uint8 (c, h, w) tensor VIEW for Encoder.submit_planar (fpng_amd_image_planar), from
    its strides and data_ptr() alone (the device is not touched, so CPU tensors work too): c = 3 or 4 planes, stride(2) == 1,
    stride(1) the row pitch, stride(0) the plane pitch -- a contiguous CHW tensor, nchw[i], rgba_chw[:3], a crop chw[:, y0:y1, x0:x1].

    order: how the planes are stored -- "rgb" or, planes stored B, G, R, "bgr" (the base is then the last plane and the plane pitch
    negative); for c = 4 "rgba" or "abgr" (one pitch cannot say another order).  bottom_up: the tensor's row 0 is the image's BOTTOM
    row.  Refused: other dtypes and ranks, stride(2) != 1 (an interleaved view: that is submit_ex's), rows or planes that overlap,
    stride 0."""
    return _planar_layout(t, order, bottom_up, "source_layout_planar")


def dest_layout_planar(t, order="rgb", bottom_up=False):
    """(d_pixels, row_pitch, plane_pitch) of a uint8 (c, h, w) tensor VIEW that a decode fills in place (Encoder.decode_device_planar /
    decode_batch_planar, fpng_amd_png_planar): the destination twin of source_layout_planar(), same rules.  c = 4 planes of a
    3-channel file: the A plane is filled with 0xFF; c = 3 of a 4-channel file: alpha is dropped."""
    return _planar_layout(t, order, bottom_up, "dest_layout_planar")


# torch dtype of a float destination -> FPNG_AMD_F32 / _F16 / _BF16 (fpng_amd_float_format::dtype)
FLOAT_DTYPES = {torch.float32: _lib.F32, torch.float16: _lib.F16, torch.bfloat16: _lib.BF16}


def normalize_constants(mean, std, max_value=255.0):
    """(scale[4], bias[4]) as float32 arrays for the float decode calls: an element is fmaf(byte, scale[c], bias[c]), and with
    scale[c] = 1 / (max_value * std[c]), bias[c] = -mean[c] / std[c] that is (byte / max_value - mean[c]) / std[c] -- torchvision's
    ToTensor() + Normalize(mean, std).  Computed in float64, rounded once; channels that mean / std do not name (alpha, usually)
    get 1 / max_value and 0: plain [0, 1] values."""
    mean, std = np.atleast_1d(np.asarray(mean, dtype=np.float64)), np.atleast_1d(np.asarray(std, dtype=np.float64))
    if mean.ndim != 1 or mean.shape != std.shape or mean.size > 4:
        raise ValueError("normalize_constants: mean and std are sequences of the same length, at most 4")
    if not (np.all(np.isfinite(mean)) and np.all(np.isfinite(std)) and np.all(std != 0) and np.isfinite(max_value) and max_value != 0):
        raise ValueError("normalize_constants: finite mean, finite non-zero std and max_value")
    scale, bias = np.full(4, 1.0 / float(max_value)), np.zeros(4)
    scale[: mean.size], bias[: mean.size] = 1.0 / (float(max_value) * std), -mean / std
    return scale.astype(np.float32), bias.astype(np.float32)


def dest_layout_float(t, order="rgb", bottom_up=False):
    """(d_pixels, row_pitch, plane_pitch, dtype code) of a float32 / float16 / bfloat16 (c, h, w) tensor VIEW that a float decode
    fills in place (Encoder.decode_device_float / decode_batch_float): dest_layout_planar()'s rules on strides counted in
    ELEMENTS -- contiguous CHW, nchw[i], chw4[:3], crops, padded rows, order "bgr" / "abgr", bottom_up -- and its refusals, plus
    any other dtype; the pitches come back in BYTES, as fpng_amd_png_planar takes them."""
    if not isinstance(t, torch.Tensor) or t.dtype not in FLOAT_DTYPES:
        raise ValueError("dest_layout_float: a float32, float16 or bfloat16 tensor shaped (c, h, w)")
    ptr, rp, pp = _planar_layout(t, order, bottom_up, "dest_layout_float", elem=t.element_size())
    return ptr, rp, pp, FLOAT_DTYPES[t.dtype]


def dest_layout_hwc(t, order="rgb", bottom_up=False):
    """(d_pixels, row_pitch, pixel_elems, flags, dtype code or None) of an (h, w, c) tensor VIEW -- uint8 (dtype code None) or
    float32 / float16 / bfloat16 -- that Encoder.decode_device_views_hwc / decode_batch_views_hwc fill in place
    (fpng_amd_view_dest_hwc), from its strides and data_ptr() alone (the device is not touched, so CPU tensors work too).

    c is 3 or 4 and stride(2) == 1; stride(1), the pixel, is c elements, or 4 with c = 3 ([..., :3] of an RGBA tensor: the fourth
    element of every pixel is never written, and the view starts on a multiple of 4 elements: [..., 1:] is refused; with w == 1 any
    stride(1) is accepted); stride(0) at least the row's span, rows that
    overlap and stride 0 refused.  A contiguous HWC tensor, a crop hwc[y0:y1, x0:x1], and -- what the call exists for -- the
    permute(1, 2, 0) of x[i] of a torch.channels_last batch x.  order: "rgb" / "bgr" for c = 3, "rgba" / "abgr" for c = 4 ("rgb"
    with 4 means "rgba"); bottom_up: the tensor's row 0 is the image's BOTTOM row.  Strides count elements; the pitch comes back
    in BYTES."""
    who = "dest_layout_hwc"
    if not isinstance(t, torch.Tensor) or (t.dtype != torch.uint8 and t.dtype not in FLOAT_DTYPES) or t.dim() != 3:
        raise ValueError(f"{who}: a uint8, float32, float16 or bfloat16 tensor shaped (h, w, c)")
    h, w, c = t.shape
    if c not in (3, 4) or h < 1 or w < 1:
        raise ValueError(f"{who}: {c} channels (3 or 4), {w} x {h}")
    if t.stride(2) != 1:
        raise ValueError(f"{who}: the channels of a pixel must be adjacent elements (stride(2) == 1); stride(2) == {t.stride(2)} is a planar "
                         "view -- describe it as (c, h, w) and use decode_device_views")
    px = t.stride(1) if w > 1 else c
    if px != c and not (px == 4 and c == 3):
        raise ValueError(f"{who}: pixel stride {t.stride(1)} ({c} elements" + (" or 4" if c == 3 else "") + ")")
    order = order.lower()
    if c == 4 and order == "rgb":
        order = "rgba"
    if order not in (("rgb", "bgr") if c == 3 else ("rgba", "abgr")):
        raise ValueError(f"{who}: order {order!r} for {c} channels -- " + ("'rgb' or 'bgr'" if c == 3 else "'rgba' or 'abgr'"))
    rp, span = t.stride(0), (w - 1) * px + c
    if h > 1 and rp < span:
        raise ValueError(f"{who}: row stride {rp} < (w - 1) * pixel stride + c = {span} (rows overlap, or stride 0)")
    if h == 1:
        rp = 0  # (one row: no pitch)
    e = t.element_size()
    ptr, rp = t.data_ptr(), rp * e
    if px != c and ptr % (4 * e):
        raise ValueError(f"{who}: a 3-channel view of 4-element pixels starts at the pixel's first element ([..., :3], not [..., 1:])")
    if bottom_up and h > 1:
        ptr, rp = ptr + (h - 1) * rp, -rp
    return ptr, rp, px, (0 if order[0] == "r" else _lib.HWC_REVERSED), FLOAT_DTYPES.get(t.dtype)


def denormalize_constants(mean, std, max_value=255.0):
    """(scale[4], bias[4]) as float32 arrays for the float encode calls, the inverse of normalize_constants(): a byte is
    rint(fmaf(x, scale[c], bias[c])) clamped to [0, 255], and with scale[c] = max_value * std[c], bias[c] = max_value * mean[c] that
    is (x * std[c] + mean[c]) * max_value -- what undoes torchvision's Normalize(mean, std) and ToTensor().  Computed in float64,
    rounded once; channels that mean / std do not name (alpha, usually) get max_value and 0: plain [0, 1] values."""
    mean, std = np.atleast_1d(np.asarray(mean, dtype=np.float64)), np.atleast_1d(np.asarray(std, dtype=np.float64))
    if mean.ndim != 1 or mean.shape != std.shape or mean.size > 4:
        raise ValueError("denormalize_constants: mean and std are sequences of the same length, at most 4")
    if not (np.all(np.isfinite(mean)) and np.all(np.isfinite(std)) and np.all(std != 0) and np.isfinite(max_value) and max_value != 0):
        raise ValueError("denormalize_constants: finite mean, finite non-zero std and max_value")
    scale, bias = np.full(4, float(max_value)), np.zeros(4)
    scale[: mean.size], bias[: mean.size] = float(max_value) * std, float(max_value) * mean
    return scale.astype(np.float32), bias.astype(np.float32)


def source_layout_float(t, order="rgb", bottom_up=False):
    """(d_pixels, row_pitch, plane_pitch, dtype code) of a float32 / float16 / bfloat16 (c, h, w) tensor VIEW for
    Encoder.submit_float (fpng_amd_encode_submit_planar_float): source_layout_planar()'s rules on strides counted in ELEMENTS --
    contiguous CHW, nchw[i], chw4[:3], crops, padded rows, order "bgr" / "abgr", bottom_up -- and its refusals, plus any other
    dtype; the pitches come back in BYTES, as fpng_amd_image_planar takes them.  The device is not touched: CPU tensors work too."""
    if not isinstance(t, torch.Tensor) or t.dtype not in FLOAT_DTYPES:
        raise ValueError("source_layout_float: a float32, float16 or bfloat16 tensor shaped (c, h, w)")
    ptr, rp, pp = _planar_layout(t, order, bottom_up, "source_layout_float", elem=t.element_size())
    return ptr, rp, pp, FLOAT_DTYPES[t.dtype]


def _float_constants(who, make, mean, std, scale, bias):
    """scale[4], bias[4] of a float call from its mean / std or scale / bias arguments; make: normalize_constants or
    denormalize_constants, whose values for no channels named are the defaults"""
    if (mean is None) != (std is None) or (mean is not None and (scale is not None or bias is not None)):
        raise ValueError(f"{who}: mean and std together, or scale and / or bias, or neither")
    if mean is not None:
        sc, bi = make(mean, std)
    else:
        sc, bi = make([], [])
        for dst, src, what in ((sc, scale, "scale"), (bi, bias, "bias")):
            if src is not None:
                v = np.atleast_1d(np.asarray(src, dtype=np.float32))
                if v.ndim != 1 or not 1 <= v.size <= 4:
                    raise ValueError(f"{who}: {what} has 1 to 4 values")
                dst[: v.size] = v
    if not (np.all(np.isfinite(sc)) and np.all(np.isfinite(bi))):
        raise ValueError(f"{who}: scale and bias must be finite")
    return sc, bi


def crop_tiles(file_w, file_h, crop):
    """fpng_amd_decode_crop_tiles: (n_segments, first_col_block, n_col_blocks) -- the tiles of the decoder's pixel pass (segments of
    48 rows x column blocks of 256 pixels) that a crop (x, y, w, h) of a file_w x file_h file needs: segments 0 .. n_segments - 1
    of the column blocks first_col_block .. first_col_block + n_col_blocks - 1.  No GPU needed.  An empty crop or one that
    leaves the image raises FpngAmdError (FPNG_AMD_ERR_INVALID_ARG)."""
    x, y, w, h = (int(v) for v in crop)
    c = _lib.Crop(x, y, w, h)
    nseg, first, ncb = C.c_uint32(), C.c_uint32(), C.c_uint32()
    check(_lib.load().fpng_amd_decode_crop_tiles(int(file_w), int(file_h), C.byref(c), C.byref(nseg), C.byref(first), C.byref(ncb)))
    return nseg.value, first.value, ncb.value


FILTERS = {"bilinear": FILTER_BILINEAR, "bicubic": FILTER_BICUBIC}


def _filter_id(who, f):
    """a filter's name ("bilinear", "bicubic") or FILTER_* value -> the value"""
    if isinstance(f, str):
        if f not in FILTERS:
            raise ValueError(f"{who}: filter {f!r} ({', '.join(sorted(FILTERS))})")
        return FILTERS[f]
    f = int(f)
    if not 0 <= f <= 0xFFFFFFFF:
        raise ValueError(f"{who}: filter {f}")
    return f  # (an unknown value: the library's refusal)


def resize_weights(in_size, out_size, filter="bilinear"):
    """fpng_amd_resize_weights(_filter): (first, count, weights) of one axis of decode_device_resize() / decode_device_resize_view()
    -- numpy arrays first[out_size], count[out_size] (uint32) and weights[out_size, 65] (int32, 22-bit fixed point, 0 behind a row's
    count): output sample o is clamp((2^21 + sum_t in[first[o] + t] * weights[o, t]) >> 22, 0, 255).  filter: "bilinear" (the
    default) or "bicubic", whose weights may be negative.  The text the kernel runs; no GPU needed.  A size of 0 or in_size >
    32 * out_size (bicubic: 16 * out_size) raises FpngAmdError (FPNG_AMD_ERR_INVALID_ARG)."""
    in_size, out_size = int(in_size), int(out_size)
    if not (0 <= in_size <= 0xFFFFFFFF and 0 <= out_size <= 0xFFFFFFFF):
        raise ValueError(f"resize_weights: sizes {in_size} -> {out_size} (32 bits, not negative)")
    fid = _filter_id("resize_weights", filter)
    first, count = np.zeros(max(out_size, 1), dtype=np.uint32), np.zeros(max(out_size, 1), dtype=np.uint32)
    weights = np.zeros((max(out_size, 1), _lib.RESIZE_MAX_TAPS), dtype=np.int32)
    ptrs = (first.ctypes.data_as(C.POINTER(C.c_uint32)), count.ctypes.data_as(C.POINTER(C.c_uint32)), weights.ctypes.data_as(C.POINTER(C.c_int32)))
    if fid == FILTER_BILINEAR:
        check(_lib.load().fpng_amd_resize_weights(in_size, out_size, *ptrs))
    else:
        check(_lib.load().fpng_amd_resize_weights_filter(in_size, out_size, fid, *ptrs))
    return first, count, weights


def _view_record(who, full, window, filter, mirror, rec=None):
    """(full_w, full_h), (x, y, w, h) or None for the whole, a filter, a mirror flag -> an fpng_amd_resize_view"""
    fw, fh = (int(v) for v in full)
    x, y, w, h = (0, 0, fw, fh) if window is None else (int(v) for v in window)
    if min(fw, fh, x, y, w, h) < 0 or max(fw, fh, x, y, w, h) > 0xFFFFFFFF:
        raise ValueError(f"{who}: full {tuple(full)}, window {window} (values of 32 bits, not negative)")
    rec = _lib.ResizeView() if rec is None else rec
    rec.full_w, rec.full_h, rec.x, rec.y, rec.w, rec.h = fw, fh, x, y, w, h
    rec.flags, rec.filter = (RESIZE_MIRROR if mirror else 0), _filter_id(who, filter)
    return rec


def resize_view_source(crop, full, window=None, filter="bilinear"):
    """fpng_amd_resize_view_source: the box (x, y, w, h) of the file's pixels that the taps of a view reach -- the window (x, y, w,
    h) (None: the whole) of the crop (x, y, w, h) resized to full = (full_w, full_h) by `filter` -- which is what the crop stage of
    decode_device_resize_view() decodes: crop_tiles(file_w, file_h, box) names the tiles that run.  No GPU needed.  Whatever the
    call refuses in a record raises FpngAmdError (FPNG_AMD_ERR_INVALID_ARG)."""
    c, box = _crop_record("resize_view_source", crop), _lib.Crop()
    v = _view_record("resize_view_source", full, window, filter, False)
    check(_lib.load().fpng_amd_resize_view_source(C.byref(c), C.byref(v), C.byref(box)))
    return box.x, box.y, box.w, box.h


def _is_ints(v, k):
    return not isinstance(v, (str, bytes)) and hasattr(v, "__len__") and len(v) == k and all(isinstance(a, (int, np.integer)) for a in v)


# what one value of a view's argument looks like (make_decode_batch_views: once for all, per file or per view)
_VIEW_ARG = {"full sizes": lambda v: _is_ints(v, 2), "windows": lambda v: v is None or _is_ints(v, 4),
             "filters": lambda v: isinstance(v, (str, int, np.integer)), "mirror flags": lambda v: isinstance(v, (bool, int, np.bool_)),
             "plane orders": lambda v: isinstance(v, str), "bottom_up flags": lambda v: isinstance(v, (bool, np.bool_))}


def _per_view(who, counts, v, what):
    """an argument of the views call -> a list per file of a value per view.  v: one value (for all views of all files), a
    sequence with an entry per file, each entry one value (for the file's views) or a sequence with a value per view"""
    one = _VIEW_ARG[what]
    if one(v):
        return [[v] * c for c in counts]
    vs = list(v)
    if len(vs) != len(counts):
        raise ValueError(f"{who}: {len(counts)} files, {len(vs)} {what}")
    out = []
    for i, (c, f) in enumerate(zip(counts, vs)):
        fs = [f] * c if one(f) else list(f)
        if len(fs) != c or not all(one(a) for a in fs):
            raise ValueError(f"{who}: file {i} has {c} views, its {what}: {f!r}")
        out.append(fs)
    return out


def _crop_record(who, crop, rec=None):
    x, y, w, h = (int(v) for v in crop)
    if min(x, y, w, h) < 0 or max(x, y, w, h) > 0xFFFFFFFF:
        raise ValueError(f"{who}: crop {tuple(crop)} (four values of 32 bits, not negative)")
    rec = _lib.Crop() if rec is None else rec
    rec.x, rec.y, rec.w, rec.h = x, y, w, h
    return rec


def views_source(crops, fulls, windows=None, filters="bilinear"):
    """fpng_amd_views_source: the ONE box (x, y, w, h) of a file's pixels that decode_device_views() decodes for a file with these
    views -- the bounding rectangle of resize_view_source(crops[k], fulls[k], windows[k], filters[k]).  crops: an (x, y, w, h) per
    view; fulls, windows, filters: one per view, or one for all.  crop_tiles(file_w, file_h, box) names the tiles that run.  No GPU
    needed.  Whatever the call refuses in a record, and no view at all, raise FpngAmdError (FPNG_AMD_ERR_INVALID_ARG)."""
    who = "views_source"
    count = len(crops)
    fulls, windows, filters = (_per_view(who, [count], [v] if _VIEW_ARG[what](v) else [list(v)], what)[0]
                               for v, what in ((fulls, "full sizes"), (windows, "windows"), (filters, "filters")))
    carr, varr, box = (_lib.Crop * max(count, 1))(), (_lib.ResizeView * max(count, 1))(), _lib.Crop()
    for k in range(count):
        _crop_record(who, crops[k], carr[k])
        _view_record(who, fulls[k], windows[k], filters[k], False, varr[k])
    check(_lib.load().fpng_amd_views_source(carr, varr, count, C.byref(box)))
    return box.x, box.y, box.w, box.h


_LUMA = (0.2989, 0.587, 0.114)  # torchvision's rgb_to_grayscale
_RGB_TO_YIQ = ((0.299, 0.587, 0.114), (0.595716, -0.274453, -0.321263), (0.211456, -0.522591, 0.311135))  # (rows I and Q sum to 0: gray has none of either)


def color_matrix(brightness=1.0, contrast=1.0, saturation=1.0, hue=0.0, contrast_center=128.0):
    """The (3, 4) float32 matrix of fpng_amd_view_color (row c: coefficients of R, G, B and a constant, in byte units) of
    ColorJitter-style factors, composed in float64 -- brightness first, then contrast, saturation, hue -- and rounded once:
        brightness  x -> b * x
        contrast    x -> k * (x - contrast_center) + contrast_center     (about a FIXED centre, not the image's own mean)
        saturation  x -> s * x + (1 - s) * L(x),  L = 0.2989 R + 0.587 G + 0.114 B (torchvision's luma); 0: RandomGrayscale's output
        hue         a rotation by `hue` turns (torchvision's range -0.5 .. 0.5) of the I, Q plane of YIQ, positive from red towards
                    yellow and green as torchvision's; 0 is exactly no step
    The defaults give exactly the identity.  No clamp between the steps: the decoder clamps once, after the matrix.  The matrix is
    the contract, this helper a convenience: for another order or another transform, multiply your own."""
    m = np.eye(4, dtype=np.float64)

    def step(a, const=(0.0, 0.0, 0.0)):
        nonlocal m
        t = np.eye(4, dtype=np.float64)
        t[:3, :3], t[:3, 3] = a, const
        m = t @ m

    b, k, sat, turn, center = float(brightness), float(contrast), float(saturation), float(hue), float(contrast_center)
    step(np.eye(3) * b)
    step(np.eye(3) * k, [(1.0 - k) * center] * 3)
    step(np.eye(3) * sat + (1.0 - sat) * np.array([_LUMA] * 3, dtype=np.float64))
    if turn != 0.0:
        yiq = np.array(_RGB_TO_YIQ, dtype=np.float64)
        co, si = np.cos(2.0 * np.pi * turn), np.sin(2.0 * np.pi * turn)
        step(np.linalg.inv(yiq) @ np.array([[1.0, 0.0, 0.0], [0.0, co, si], [0.0, -si, co]]) @ yiq)
    return np.ascontiguousarray(m[:3] + 0.0, dtype=np.float32)  # (+ 0.0: no negative zero)


def _color_record(who, m, rec=None):
    a = np.asarray(m, dtype=np.float32)
    if a.shape != (3, 4):
        raise ValueError(f"{who}: a colour matrix is (3, 4) -- per row the coefficients of R, G, B and a constant -- not {a.shape}")
    rec = _lib.ViewColor() if rec is None else rec
    for c in range(3):
        for k in range(4):
            rec.m[c][k] = float(a[c, k])
    return rec


def _color_records(who, counts, color):
    """the color= argument of the views calls -> fpng_amd_view_color[sum(counts)]: one (3, 4) array-like for all views, or a list per
    file of a list per view"""
    arr = (_lib.ViewColor * max(sum(counts), 1))()
    try:
        one = np.asarray(color, dtype=np.float32)
    except (ValueError, TypeError):
        one = None
    if one is not None and one.shape == (3, 4):
        for at in range(sum(counts)):
            _color_record(who, one, arr[at])
        return arr
    if isinstance(color, np.ndarray) or not hasattr(color, "__len__"):
        raise ValueError(f"{who}: color is one (3, 4) matrix for all views, or a list per file of a (3, 4) matrix per view")
    if len(color) != len(counts):
        raise ValueError(f"{who}: {len(counts)} files, {len(color)} lists of colour matrices")
    at = 0
    for i, (c, ms) in enumerate(zip(counts, color)):
        if isinstance(ms, np.ndarray) and ms.ndim != 3 or not hasattr(ms, "__len__") or len(ms) != c:
            raise ValueError(f"{who}: file {i} has {c} views, its colour matrices: {np.shape(ms)}")
        for m in ms:
            _color_record(f"{who}: file {i}", m, arr[at])
            at += 1
    return arr


def color_apply(matrix, rgb_bytes):
    """fpng_amd_color_apply, the host twin of the colour step (no GPU): rgb_bytes (..., 3) uint8 -> (..., 3) float32, the u_c of the
    rule -- fminf(fmaxf(fmaf(m[c][2], b, fmaf(m[c][1], g, fmaf(m[c][0], r, m[c][3]))), 0), 255) -- that the kernel computes for
    those bytes under `matrix` (3, 4)."""
    rec = _color_record("color_apply", matrix)
    px = np.ascontiguousarray(rgb_bytes, dtype=np.uint8)
    if px.ndim < 1 or px.shape[-1] != 3:
        raise ValueError(f"color_apply: rgb_bytes is (..., 3) uint8, not {px.shape}")
    out = np.empty(px.shape, dtype=np.float32)
    fn, flat, oflat = _lib.load().fpng_amd_color_apply, px.reshape(-1, 3), out.reshape(-1, 3)
    rgb, u = (C.c_uint8 * 3)(), (C.c_float * 3)()
    for k in range(flat.shape[0]):
        rgb[0], rgb[1], rgb[2] = flat[k]
        fn(C.byref(rec), C.byref(rgb), C.byref(u))
        oflat[k] = u[0], u[1], u[2]
    return out


def view_post(blur=None, solarize=None, posterize=None):
    """The fpng_amd_view_post record of one view of the views calls' post= argument: what torchvision's GaussianBlur, RandomSolarize
    and RandomPosterize do to a uint8 image, behind the colour matrix and in front of the normalisation.  blur: None, or (kernel_size,
    sigma) with an odd kernel_size of 3 .. 33 (radius (kernel_size - 1) / 2) and sigma > 0; solarize: None, or the threshold 0 .. 255
    (bytes >= it are inverted); posterize: None, or the bits 0 .. 8 that are kept.  All None: the view is the colour call's,
    untouched.  The caller draws the probabilities and the sigma; the record is the contract."""
    rec = _lib.ViewPost()
    if blur is not None:
        try:
            ks, sigma = blur
        except (TypeError, ValueError):
            raise ValueError("view_post: blur is (kernel_size, sigma)") from None
        if int(ks) != ks or int(ks) % 2 != 1 or not 3 <= int(ks) <= 2 * _lib.BLUR_MAX_RADIUS + 1:
            raise ValueError(f"view_post: a blur's kernel_size is odd, 3 .. {2 * _lib.BLUR_MAX_RADIUS + 1}, not {ks}")
        rec.flags |= _lib.POST_BLUR
        rec.blur_radius, rec.blur_sigma = (int(ks) - 1) // 2, float(sigma)
    if solarize is not None:
        if int(solarize) != solarize or not 0 <= int(solarize) <= 255:
            raise ValueError(f"view_post: a solarize threshold is an integer 0 .. 255, not {solarize}")
        rec.flags |= _lib.POST_SOLARIZE
        rec.solarize_threshold = int(solarize)
    if posterize is not None:
        if int(posterize) != posterize or not 0 <= int(posterize) <= 8:
            raise ValueError(f"view_post: posterize keeps 0 .. 8 bits, not {posterize}")
        rec.flags |= _lib.POST_POSTERIZE
        rec.posterize_bits = int(posterize)
    return rec


_WARP_FILTERS = {"nearest": _lib.WARP_AFFINE, "bilinear": _lib.WARP_AFFINE | _lib.WARP_BILINEAR}


def view_warp(matrix=None, filter="nearest", fill=0):
    """The fpng_amd_view_warp record of one view of the views calls' warp= argument: matrix, the six coefficients of Pillow's
    Image.transform(size, Image.AFFINE, matrix) -- output pixel centre -> source position, xs = a0 (x + .5) + a1 (y + .5) + a2,
    ys = a3 (x + .5) + a4 (y + .5) + a5; affine_matrix() makes them -- sampled "nearest" or "bilinear" as Pillow samples, with `fill`
    (one byte for all four channels, or a list of up to four, per FILE channel; a list's missing fourth is 255) outside the window.  matrix None: the view
    is the post call's, untouched.  The caller draws the angles; the record is the contract."""
    rec = _lib.ViewWarp()
    if matrix is None:
        return rec
    try:
        a = [float(v) for v in matrix]
    except (TypeError, ValueError):
        a = []
    if len(a) != 6:
        raise ValueError("view_warp: matrix is the six coefficients (a0 .. a5) of Pillow's AFFINE transform")
    if filter not in _WARP_FILTERS:
        raise ValueError(f"view_warp: filter is 'nearest' or 'bilinear', not {filter!r}")
    fills = list(fill) if hasattr(fill, "__len__") else [fill] * 4
    if not 1 <= len(fills) <= 4 or any(int(f) != f or not 0 <= int(f) <= 255 for f in fills):
        raise ValueError(f"view_warp: fill is one byte 0 .. 255 or up to four of them, not {fill}")
    if len(fills) < 3:
        fills += [fills[-1]] * (3 - len(fills))
    if len(fills) < 4:
        fills.append(255)
    rec.flags = _WARP_FILTERS[filter]
    for k in range(6):
        rec.a[k] = a[k]
    for k in range(4):
        rec.fill[k] = int(fills[k])
    return rec


def view_warp_apply(warp, plane, mirror=False, fill=None):
    """fpng_amd_view_warp_apply, the host twin of the warp (no GPU): plane (h, w) uint8 -- one plane of a view's UN-MIRRORED window as
    the colour call writes it -- -> (h, w) uint8, mirrored where asked and then warped as `warp` (a view_warp() record) says.  fill:
    the byte outside (None: the record's fill[0])."""
    if not isinstance(warp, _lib.ViewWarp):
        raise ValueError("view_warp_apply: warp is what view_warp() returns")
    px = np.ascontiguousarray(plane, dtype=np.uint8)
    if px.ndim != 2 or px.size == 0:
        raise ValueError(f"view_warp_apply: plane is (h, w) uint8, not {px.shape}")
    out = np.empty_like(px)
    check(_lib.load().fpng_amd_view_warp_apply(C.byref(warp), px.shape[1], px.shape[0], 1 if mirror else 0, px.ctypes.data, out.ctypes.data,
                                               int(warp.fill[0] if fill is None else fill)))
    return out


def affine_matrix(w, h, angle=0.0, translate=(0, 0), scale=1.0, shear=(0.0, 0.0), center=None):
    """The six coefficients for view_warp() of torchvision's affine(img, angle, translate, scale, shear) on a w x h PIL image: its
    _get_inverse_affine_matrix restated in Python doubles, with the arguments that function takes -- angle and shear in degrees
    (shear: one angle for x, or (x, y)), translate in pixels, center None (the image's, (w * 0.5, h * 0.5)) or (cx, cy) in pixels.
    torchvision's rotate(img, a) hands that function -a: affine_matrix(w, h, angle=-a)."""
    shear = tuple(shear) if hasattr(shear, "__len__") else (float(shear), 0.0)
    if len(shear) != 2 or len(tuple(translate)) != 2:
        raise ValueError("affine_matrix: translate is (tx, ty), shear one angle or (sx, sy)")
    if not float(scale) > 0.0:
        raise ValueError(f"affine_matrix: scale is > 0, not {scale}")
    cx, cy = (float(w) * 0.5, float(h) * 0.5) if center is None else (float(center[0]), float(center[1]))
    tx, ty = float(translate[0]), float(translate[1])
    rot, sx, sy = math.radians(float(angle)), math.radians(float(shear[0])), math.radians(float(shear[1]))
    a = math.cos(rot - sy) / math.cos(sy)
    b = -math.cos(rot - sy) * math.tan(sx) / math.cos(sy) - math.sin(rot)
    c = math.sin(rot - sy) / math.cos(sy)
    d = -math.sin(rot - sy) * math.tan(sx) / math.cos(sy) + math.cos(rot)
    m = [v / float(scale) for v in (d, -b, 0.0, -c, a, 0.0)]
    m[2] += m[0] * (-cx - tx) + m[1] * (-cy - ty)
    m[5] += m[3] * (-cx - tx) + m[4] * (-cy - ty)
    m[2] += cx
    m[5] += cy
    return m


def view_tone(autocontrast=False, equalize=False, contrast=None):
    """The fpng_amd_view_tone record of one view of the views calls' tone= argument: at most ONE of autocontrast
    (ImageOps.autocontrast(img), cutoff 0), equalize (ImageOps.equalize(img)) and contrast=factor
    (ImageEnhance.Contrast(img).enhance(factor): factor finite and >= 0, rounded to fp32 once) -- each a statistic of the whole view,
    a table per channel and a point operation, behind the colour matrix and the warp and in front of the blur, solarize and
    posterize.  None of them: the view is the warp call's, untouched.  The caller draws the operation; the record is the contract."""
    if bool(autocontrast) + bool(equalize) + (contrast is not None) > 1:
        raise ValueError("view_tone: at most one of autocontrast, equalize and contrast (two tone operations on one view are not offered)")
    rec = _lib.ViewTone()
    if autocontrast:
        rec.op = _lib.TONE_AUTOCONTRAST
    elif equalize:
        rec.op = _lib.TONE_EQUALIZE
    elif contrast is not None:
        try:
            with np.errstate(over="ignore"):
                factor = float(np.float32(contrast))
        except (TypeError, ValueError):
            raise ValueError(f"view_tone: contrast is a number, not {contrast!r}") from None
        if not math.isfinite(factor) or factor < 0.0:
            raise ValueError(f"view_tone: contrast is finite and >= 0, not {contrast}")
        rec.op, rec.factor = _lib.TONE_CONTRAST, factor
    return rec


def _view_records(who, counts, arg, cls, noun, wrong=None):
    """the `noun`= argument of the views calls (post, warp, tone, enhance) -> cls[sum(counts)]: one record (view_<noun>() makes them)
    for all views, a list with one per file, or a list per file of one per view.  wrong: what to say of an entry that is no such
    record, where the argument has a wording of its own"""
    total = sum(counts)
    arr = (cls * max(total, 1))()

    def put(at, rec):
        if not isinstance(rec, cls):
            raise ValueError(f"{who}: {wrong or f'{noun} takes what view_{noun}() returns'}, not {type(rec).__name__}")
        C.memmove(C.byref(arr, at * C.sizeof(cls)), C.byref(rec), C.sizeof(cls))

    if isinstance(arg, cls):
        for at in range(total):
            put(at, arg)
        return arr
    if not hasattr(arg, "__len__") or len(arg) != len(counts):
        raise ValueError(f"{who}: {noun} is one view_{noun}() record for all views, or a list with an entry per file ({len(counts)}), each one record or a list of one per view")
    at = 0
    for i, (c, recs) in enumerate(zip(counts, arg)):
        if isinstance(recs, cls):
            recs = [recs] * c
        if not hasattr(recs, "__len__") or len(recs) != c:
            raise ValueError(f"{who}: file {i} has {c} views, not {len(recs) if hasattr(recs, '__len__') else 1} {noun} records")
        for rec in recs:
            put(at, rec)
            at += 1
    return arr


def view_tone_lut(tone, hist):
    """fpng_amd_view_tone_lut, the host twin of the tone tables (no GPU): hist (4, 256) counts -- of R, G, B and of Pillow's L -- ->
    the (3, 256) uint8 tables of `tone` (a view_tone() record)."""
    if not isinstance(tone, _lib.ViewTone):
        raise ValueError("view_tone_lut: tone is what view_tone() returns")
    h = np.asarray(hist)
    if h.shape != (4, 256) or h.dtype.kind not in "iu" or (h.size and (h.min() < 0 or h.max() > 0xFFFFFFFF)):
        raise ValueError("view_tone_lut: hist is (4, 256) counts that fit uint32")
    h = np.ascontiguousarray(h, dtype=np.uint32)
    lut = np.empty((3, 256), dtype=np.uint8)
    check(_lib.load().fpng_amd_view_tone_lut(C.byref(tone), h.ctypes.data, lut.ctypes.data))
    return lut


def view_tone_apply(tone, planes):
    """fpng_amd_view_tone_apply, the host twin of the tone stage (no GPU): planes (3, h, w) uint8 -- a view's window as the post stage
    loads it -- -> (3, h, w) uint8 through the histograms and tables of `tone` (a view_tone() record)."""
    if not isinstance(tone, _lib.ViewTone):
        raise ValueError("view_tone_apply: tone is what view_tone() returns")
    px = np.asarray(planes)
    if px.dtype != np.uint8 or px.ndim != 3 or px.shape[0] != 3 or px.size == 0:
        raise ValueError(f"view_tone_apply: planes is (3, h, w) uint8, not {px.shape} {px.dtype}")
    px = np.ascontiguousarray(px)
    out = np.empty_like(px)
    check(_lib.load().fpng_amd_view_tone_apply(C.byref(tone), px.shape[2], px.shape[1], px.ctypes.data, out.ctypes.data))
    return out


def view_enhance(brightness=None, color=None, sharpness=None):
    """The fpng_amd_view_enhance record of one view of the views calls' enhance= argument: at most ONE of brightness=factor
    (ImageEnhance.Brightness(img).enhance(factor)), color=factor (ImageEnhance.Color) and sharpness=factor (ImageEnhance.Sharpness)
    -- factor finite and >= 0, rounded to fp32 once; 1 is the identity -- each Pillow's blend of a degenerate image (black, the
    view's grey image, its SMOOTH-filtered image) and the view, behind the tone operation and in front of the blur, solarize and
    posterize.  None of them: the view is the tone call's, untouched.  The caller draws the operation; the record is the contract."""
    given = [(op, name, f) for op, name, f in ((_lib.ENHANCE_BRIGHTNESS, "brightness", brightness), (_lib.ENHANCE_COLOR, "color", color),
                                               (_lib.ENHANCE_SHARPNESS, "sharpness", sharpness)) if f is not None]
    if len(given) > 1:
        raise ValueError("view_enhance: at most one of brightness, color and sharpness (two enhance operations on one view are not offered)")
    rec = _lib.ViewEnhance()
    for op, name, f in given:
        try:
            with np.errstate(over="ignore"):
                factor = float(np.float32(f))
        except (TypeError, ValueError):
            raise ValueError(f"view_enhance: {name} is a number, not {f!r}") from None
        if not math.isfinite(factor) or factor < 0.0:
            raise ValueError(f"view_enhance: {name} is finite and >= 0, not {f}")
        rec.op, rec.factor = op, factor
    return rec


def view_enhance_apply(enhance, planes):
    """fpng_amd_view_enhance_apply, the host twin of the enhance stage (no GPU): planes (3, h, w) uint8 -- what the tone stage hands
    on -- -> (3, h, w) uint8 blended against the degenerate image of `enhance` (a view_enhance() record)."""
    if not isinstance(enhance, _lib.ViewEnhance):
        raise ValueError("view_enhance_apply: enhance is what view_enhance() returns")
    px = np.asarray(planes)
    if px.dtype != np.uint8 or px.ndim != 3 or px.shape[0] != 3 or px.size == 0:
        raise ValueError(f"view_enhance_apply: planes is (3, h, w) uint8, not {px.shape} {px.dtype}")
    px = np.ascontiguousarray(px)
    out = np.empty_like(px)
    check(_lib.load().fpng_amd_view_enhance_apply(C.byref(enhance), px.shape[2], px.shape[1], px.ctypes.data, out.ctypes.data))
    return out


RESAMPLE_FILTERS = {None: 0, "nearest": _lib.RESAMPLE_NEAREST, "box": _lib.RESAMPLE_BOX, "hamming": _lib.RESAMPLE_HAMMING, "lanczos": _lib.RESAMPLE_LANCZOS}


def view_resample(filter=None):
    """The fpng_amd_view_resample record of one view of the views calls' resample= argument: the filter the view is resized with in
    the place of its own filter= -- "nearest", "box", "hamming" or "lanczos", Pillow's Image.NEAREST, BOX, HAMMING and LANCZOS -- or
    None: the view's own (the view is then the alpha call's, untouched).  An integer is taken as an FPNG_AMD_RESAMPLE_* value."""
    rec = _lib.ViewResample()
    if isinstance(filter, (int, np.integer)) and not isinstance(filter, bool) and 0 <= int(filter) <= 0xFFFFFFFF:
        rec.filter = int(filter)  # (an unknown value: the library's refusal)
    elif isinstance(filter, (str, type(None))) and filter in RESAMPLE_FILTERS:
        rec.filter = RESAMPLE_FILTERS[filter]
    else:
        raise ValueError(f"view_resample: filter is None, 'nearest', 'box', 'hamming' or 'lanczos', not {filter!r}")
    return rec


def _resample_arg(arg):
    """the resample= argument with its names (and None entries below the top) as view_resample() records"""
    one = lambda v: v is None or isinstance(v, (str, int, np.integer))
    if one(arg):
        return view_resample(arg)
    if isinstance(arg, _lib.ViewResample) or not hasattr(arg, "__len__"):
        return arg
    return [view_resample(f) if one(f) else f if isinstance(f, _lib.ViewResample) or not hasattr(f, "__len__") else [view_resample(v) if one(v) else v for v in f] for f in arg]


def resample_weights(in_size, out_size, filter):
    """fpng_amd_resample_weights: resize_weights() for the RESAMPLE filters "nearest", "box", "hamming" and "lanczos" -> (first, count,
    weights).  "nearest": count 1, weight 2^22, first = Pillow's index.  The text the kernels run; no GPU needed.  A size of 0 or one
    past the filter's limit (in_size <= 32 * out_size; lanczos: 3 * in_size <= 32 * out_size) raises FpngAmdError."""
    in_size, out_size = int(in_size), int(out_size)
    if not (0 <= in_size <= 0xFFFFFFFF and 0 <= out_size <= 0xFFFFFFFF):
        raise ValueError(f"resample_weights: sizes {in_size} -> {out_size} (32 bits, not negative)")
    fid = view_resample(filter).filter
    first, count = np.zeros(max(out_size, 1), dtype=np.uint32), np.zeros(max(out_size, 1), dtype=np.uint32)
    weights = np.zeros((max(out_size, 1), _lib.RESIZE_MAX_TAPS), dtype=np.int32)
    check(_lib.load().fpng_amd_resample_weights(in_size, out_size, fid, first.ctypes.data_as(C.POINTER(C.c_uint32)), count.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                weights.ctypes.data_as(C.POINTER(C.c_int32))))
    return first, count, weights


def resample_view_source(crop, full, window=None, filter="bilinear", resample=None):
    """fpng_amd_resample_view_source: resize_view_source() of a view whose RESAMPLE record is view_resample(resample) (a name, None or
    a record).  No GPU needed."""
    c, box = _crop_record("resample_view_source", crop), _lib.Crop()
    v = _view_record("resample_view_source", full, window, filter, False)
    r = resample if isinstance(resample, _lib.ViewResample) else view_resample(resample)
    check(_lib.load().fpng_amd_resample_view_source(C.byref(c), C.byref(v), C.byref(r), C.byref(box)))
    return box.x, box.y, box.w, box.h


def view_alpha(op=None, background=(0, 0, 0)):
    """The fpng_amd_view_alpha record of one view of the views calls' alpha= argument: what the view does with the fourth plane of a
    4-channel file, inside the resize.  op="composite": every sample is put over the opaque `background` (R, G, B bytes) first, as
    Image.alpha_composite(Image.new("RGBA", im.size, background + (255,)), im) does, then cropped and resized; a fourth destination
    plane is 255.  op="premultiplied": Pillow's Image.resize of an RGBA image -- RGBA -> RGBa, resample, RGBa -> RGBA.  op=None: the
    view is the enhance call's, untouched (alpha resized on its own, or dropped).  On a 3-channel file every op is op None."""
    ops = {None: 0, "composite": _lib.ALPHA_COMPOSITE, "premultiplied": _lib.ALPHA_PREMULTIPLIED}
    if not (op is None or isinstance(op, str)) or op not in ops:
        raise ValueError(f"view_alpha: op is None, 'composite' or 'premultiplied', not {op!r}")
    try:
        bg = [int(b) for b in background]
        if len(bg) != 3 or any(b != f for b, f in zip(bg, background)) or not all(0 <= b <= 255 for b in bg):
            raise ValueError
    except (TypeError, ValueError):
        raise ValueError(f"view_alpha: background is three integers 0 .. 255 (R, G, B), not {background!r}") from None
    if ops[op] != _lib.ALPHA_COMPOSITE and any(bg):
        raise ValueError("view_alpha: a background goes with op='composite'")
    rec = _lib.ViewAlpha()
    rec.op = ops[op]
    for k in range(3):
        rec.background[k] = bg[k]
    return rec


def _view_alpha_twin(who, symbol, alpha, planes):
    if not isinstance(alpha, _lib.ViewAlpha):
        raise ValueError(f"{who}: alpha is what view_alpha() returns")
    px = np.asarray(planes)
    if px.dtype != np.uint8 or px.ndim != 3 or px.shape[0] != 4 or px.size == 0:
        raise ValueError(f"{who}: planes is (4, h, w) uint8, not {px.shape} {px.dtype}")
    px = np.ascontiguousarray(px)
    out = np.empty_like(px)
    check(getattr(_lib.load(), symbol)(C.byref(alpha), px.shape[2], px.shape[1], px.ctypes.data, out.ctypes.data))
    return out


def view_alpha_source(alpha, planes):
    """fpng_amd_view_alpha_source, the host twin of the alpha stage's load (no GPU): planes (4, h, w) uint8 -- a crop's four planes --
    -> (4, h, w) uint8, what the resize of a view with `alpha` (a view_alpha() record) reads: composited over the background with
    255 in the fourth plane, premultiplied, or a copy."""
    return _view_alpha_twin("view_alpha_source", "fpng_amd_view_alpha_source", alpha, planes)


def view_alpha_result(alpha, planes):
    """fpng_amd_view_alpha_result, the host twin of the alpha stage's store (no GPU): planes (4, h, w) uint8 -- the resize's four
    result planes -- -> (4, h, w) uint8, what the later stages see: divided by the fourth plane for a premultiplied view, else a copy."""
    return _view_alpha_twin("view_alpha_result", "fpng_amd_view_alpha_result", alpha, planes)


def rotate_matrix(w, h, angle):
    """The six coefficients for view_warp() that Pillow's Image.rotate(angle) (no expand, the default centre, no translate) hands to
    transform() for a w x h image, computed as Pillow computes them: the cosine and sine of -radians(angle % 360) rounded to 15
    digits, about the centre (w / 2, h / 2).  torchvision's rotate() of a PIL image calls Image.rotate; affine_matrix(w, h,
    angle=-a) is torchvision's tensor path and differs from this in the last bits."""
    cx, cy = w / 2, h / 2
    a = -math.radians(float(angle) % 360.0)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
    m[2] = m[0] * -cx + m[1] * -cy + m[2]
    m[5] = m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    return m


AUGMENT_OPS = ("Identity", "ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate", "Brightness", "Color", "Contrast", "Sharpness", "Posterize", "Solarize",
               "AutoContrast", "Equalize")


def augment_op(name, magnitude, w, h, filter="nearest", fill=0):
    """The records of ONE operation of RandAugment / TrivialAugmentWide / AutoAugment on a w x h view, as a dict of keyword arguments
    for the views calls (color= / warp= / tone= / enhance= / post=; only the keys the operation needs): `name` is one of the 14 that
    torchvision's _apply_op knows (AUGMENT_OPS) and `magnitude` what _apply_op receives, already signed.  filter and fill are the
    geometric operations' interpolation and fill."""
    m = float(magnitude)
    if name == "Identity":
        return {}
    if name == "ShearX":
        return {"warp": view_warp(affine_matrix(w, h, shear=(math.degrees(math.atan(m)), 0.0), center=(0, 0)), filter, fill)}
    if name == "ShearY":
        return {"warp": view_warp(affine_matrix(w, h, shear=(0.0, math.degrees(math.atan(m))), center=(0, 0)), filter, fill)}
    if name == "TranslateX":
        return {"warp": view_warp(affine_matrix(w, h, translate=(int(m), 0)), filter, fill)}
    if name == "TranslateY":
        return {"warp": view_warp(affine_matrix(w, h, translate=(0, int(m))), filter, fill)}
    if name == "Rotate":
        return {"warp": view_warp(rotate_matrix(w, h, m), filter, fill)}
    if name == "Brightness":
        return {"enhance": view_enhance(brightness=1.0 + m)}
    if name == "Color":
        return {"enhance": view_enhance(color=1.0 + m)}
    if name == "Sharpness":
        return {"enhance": view_enhance(sharpness=1.0 + m)}
    if name == "Contrast":
        return {"tone": view_tone(contrast=1.0 + m)}
    if name == "Posterize":
        return {"post": view_post(posterize=int(m))}
    if name == "Solarize":  # (ImageOps.solarize inverts the bytes that are not below m: those from ceil(m) on; none above 255)
        return {"post": view_post(solarize=max(math.ceil(m), 0))} if m <= 255.0 else {}
    if name == "AutoContrast":
        return {"tone": view_tone(autocontrast=True)}
    if name == "Equalize":
        return {"tone": view_tone(equalize=True)}
    raise ValueError(f"augment_op: name is one of {', '.join(AUGMENT_OPS)}, not {name!r}")


def blur_weights(radius, sigma):
    """fpng_amd_blur_weights (no GPU): the int32 weights k[0 .. radius] (2^22 fixed point) of the post calls' blur of this radius (1 ..
    16) and sigma; tap t = -radius .. radius has weight k[|t|]."""
    k = (C.c_int32 * 17)()
    check(_lib.load().fpng_amd_blur_weights(int(radius), float(sigma), C.byref(k)))
    return np.array(k[:int(radius) + 1], dtype=np.int32)


def view_post_apply(post, plane):
    """fpng_amd_view_post_apply, the host twin of the post stage (no GPU): plane (h, w) uint8 -- one colour plane of a view's window as
    the colour call writes it -- -> (h, w) uint8, blurred, solarized and posterized as `post` (a view_post() record) says."""
    if not isinstance(post, _lib.ViewPost):
        raise ValueError("view_post_apply: post is what view_post() returns")
    px = np.ascontiguousarray(plane, dtype=np.uint8)
    if px.ndim != 2 or px.size == 0:
        raise ValueError(f"view_post_apply: plane is (h, w) uint8, not {px.shape}")
    out = np.empty_like(px)
    check(_lib.load().fpng_amd_view_post_apply(C.byref(post), px.shape[1], px.shape[0], px.ctypes.data, out.ctypes.data))
    return out


def center_crop_view(file_w, file_h, resize, crop):
    """torchvision's Resize(resize) + CenterCrop(crop) of a file_w x file_h file as (crop_box, full, window) for
    decode_device_resize_view(): crop_box = the whole file, full = (full_w, full_h) with the shorter side at `resize` and the
    longer at int(resize * long / short), window = the (x, y, cw, ch) centre of it (crop: an int, or (h, w)) with
    left = int(round((full_w - cw) / 2.0)), top = int(round((full_h - ch) / 2.0)).  ValueError if the window does not fit
    (torchvision would pad)."""
    file_w, file_h, resize = int(file_w), int(file_h), int(resize)
    ch, cw = (int(crop), int(crop)) if isinstance(crop, (int, np.integer)) else (int(v) for v in crop)
    if min(file_w, file_h, resize, ch, cw) < 1:
        raise ValueError(f"center_crop_view: file {file_w} x {file_h}, resize {resize}, crop {ch} x {cw} (all at least 1)")
    if file_w <= file_h:
        full_w, full_h = resize, int(resize * file_h / file_w)
    else:
        full_w, full_h = int(resize * file_w / file_h), resize
    if cw > full_w or ch > full_h:
        raise ValueError(f"center_crop_view: a {cw} x {ch} window does not fit the resized {full_w} x {full_h} image (no padding)")
    left, top = int(round((full_w - cw) / 2.0)), int(round((full_h - ch) / 2.0))
    return (0, 0, file_w, file_h), (full_w, full_h), (left, top, cw, ch)


SYNTH_KINDS = {"noise": 0, "solid": 1, "grad": 2, "blocks": 3}


def _as_u8(data):
    if isinstance(data, np.ndarray):
        return np.ascontiguousarray(data).view(np.uint8).reshape(-1)
    return np.frombuffer(bytes(data), dtype=np.uint8)


def fpng_init(device=-1):
    check(_lib.load().fpng_amd_init(device))


def fpng_cpu_supports_sse41():
    """Kept for source compatibility; answers "is the MI355X path usable"."""
    return bool(_lib.load().fpng_amd_device_available())


def fpng_crc32(data, prev_crc32=FPNG_CRC32_INIT):
    b = _as_u8(data)
    return _lib.load().fpng_amd_crc32(b.ctypes.data, b.size, prev_crc32)


def fpng_adler32(data, adler=FPNG_ADLER32_INIT):
    b = _as_u8(data)
    return _lib.load().fpng_amd_adler32(b.ctypes.data, b.size, adler)


def crc32_combine(crc_x, crc_y, len_y):
    return _lib.load().fpng_amd_crc32_combine(crc_x, crc_y, len_y)


def adler32_combine(adler_x, adler_y, len_y):
    return _lib.load().fpng_amd_adler32_combine(adler_x, adler_y, len_y)


def max_encoded_size(w, h, num_chans):
    return _lib.load().fpng_amd_max_encoded_size(w, h, num_chans)


def pack_capacity(dims, align=16, lead=0):
    """fpng_amd_pack_capacity: the arena size with which Encoder.submit_packed() can refuse none of the images `dims` = [(w, h, c)]:
    the placement rule applied to max_encoded_size() of each."""
    n = len(dims)
    w, h, c = ((C.c_uint32 * n)(*[int(d[k]) for d in dims]) for k in range(3))
    cap = int(_lib.load().fpng_amd_pack_capacity(w, h, c, n, align, lead))
    if n and not cap:
        raise ValueError("pack_capacity: align is 0 or a power of two in 16 .. 65536, lead a multiple of 16 up to 65536")
    return cap


def pack_place(sizes, align, lead, cap, statuses=None):
    """fpng_amd_pack_place, the placement rule of packed submissions on the host: file sizes (and their statuses before placement,
    default all 0) -> ([(offset, status)], total) as the GPU decides them for an arena of `cap` bytes."""
    n = len(sizes)
    sz = (C.c_uint64 * n)(*[int(v) for v in sizes])
    st = (C.c_uint32 * n)(*[int(v) for v in statuses]) if statuses is not None else None
    off, st_out, total = (C.c_uint64 * n)(), (C.c_uint32 * n)(), C.c_uint64(0)
    check(_lib.load().fpng_amd_pack_place(sz, st, n, align, lead, cap, off, st_out, C.byref(total)))
    return list(zip(off, st_out)), total.value


# ---- renditions: resized copies of device images, encoded in one submission (fpng_amd_encode_submit_renditions) ----
RENDITION_FILTERS = _lib.RENDITION_FILTERS  # name -> FPNG_AMD_RENDITION_*
_RENDITION_ALPHA = {None: 0, "straight": 0, "premultiplied": _lib.ALPHA_PREMULTIPLIED}
_DESC_KINDS = {"image": _lib.DESC_IMAGE, "ex": _lib.DESC_EX, "planar": _lib.DESC_PLANAR, "float": _lib.DESC_PLANAR_FLOAT}


def _u32(who, what, v):
    v = int(v)
    if not 0 <= v <= 0xFFFFFFFF:
        raise ValueError(f"{who}: {what} {v}")
    return v


def rendition(image, size, box=None, filter="bilinear", alpha=None):
    """An fpng_amd_rendition record: image `image` (an index into the call's images) cropped to box = (x, y, w, h) (None: the whole
    image) and resized to size = (w, h) as Pillow's img.crop(box).resize(size, filter) does -- filter: "bilinear", "bicubic",
    "nearest", "box", "hamming" or "lanczos" (or a FPNG_AMD_RENDITION_* value).  alpha (4-channel images): None, the planes resized
    independently, or "premultiplied", Pillow's Image.resize of an RGBA image.  What the library refuses (a box outside the image, a
    scale beyond the filter's limit, ...) is refused by the call the record goes to."""
    r = _lib.Rendition()
    r.image = _u32("rendition", "image", image)
    if isinstance(filter, str):
        if filter not in RENDITION_FILTERS:
            raise ValueError(f"rendition: filter {filter!r} ({', '.join(sorted(RENDITION_FILTERS))})")
        r.filter = RENDITION_FILTERS[filter]
    else:
        r.filter = _u32("rendition", "filter", filter)
    if box is not None:
        r.box_x, r.box_y, r.box_w, r.box_h = (_u32("rendition", "box", v) for v in box)
    r.w, r.h = (_u32("rendition", "size", v) for v in size)
    if isinstance(alpha, str) or alpha is None:
        if alpha not in _RENDITION_ALPHA:
            raise ValueError(f"rendition: alpha {alpha!r} (None or 'premultiplied')")
        r.alpha_op = _RENDITION_ALPHA[alpha]
    else:
        r.alpha_op = _u32("rendition", "alpha", alpha)
    return r


def _per_image(who, n, v, one, what):
    """order / bottom_up of an encode call: one value for all images, or a sequence with one per image"""
    vs = [v] * n if isinstance(v, one) else list(v)
    if len(vs) != n:
        raise ValueError(f"{who}: {n} images, {len(vs)} {what}")
    return vs


def _source_records(who, images, kind, outs=None, order="rgb", bottom_up=False, mean=None, std=None, scale=None, bias=None):
    """The image records of every encode call: (record array of `kind`, fpng_amd_float_format or None) for tensors as
    Encoder.submit / submit_ex / submit_planar / submit_float take them, from their strides and data_ptr() alone -- CPU tensors work
    too (the host twin's).  outs: an output tensor per image, or None for records without outputs (packed calls, renditions)."""
    if kind not in _DESC_KINDS:
        raise ValueError(f"{who}: kind is one of {sorted(_DESC_KINDS)}, not {kind!r}")
    n = len(images)
    orders, ups = _per_image(who, n, order, str, "orders"), _per_image(who, n, bottom_up, bool, "bottom_up flags")
    if outs is not None and len(outs) != n:
        raise ValueError(f"{who}: {n} images, {len(outs)} outs")
    fmt = None
    if kind == "float":
        sc, bi = _float_constants(who, denormalize_constants, mean, std, scale, bias)
        dtypes = {t.dtype for t in images if isinstance(t, torch.Tensor)}
        if len(dtypes) > 1:
            raise ValueError(f"{who}: the images of one call share one dtype, not {sorted(str(d) for d in dtypes)}")
        fmt = _lib.FloatFormat()
        for k in range(4):
            fmt.scale[k], fmt.bias[k] = float(sc[k]), float(bi[k])
    elif any(v is not None for v in (mean, std, scale, bias)):
        raise ValueError(f"{who}: mean / std / scale / bias go with kind 'float'")
    if kind == "image":
        arr = (Image * n)()
        for a, im in zip(arr, images):
            if not isinstance(im, torch.Tensor) or im.dtype != torch.uint8 or im.dim() != 3 or not im.is_contiguous():
                raise ValueError(f"{who}: kind 'image' takes contiguous uint8 tensors shaped (h, w, c)")
            a.d_pixels, (a.h, a.w, a.num_chans) = im.data_ptr(), im.shape
    elif kind == "ex":
        arr = (ImageEx * n)()
        for a, im, o, up in zip(arr, images, orders, ups):
            a.d_pixels, a.row_pitch, a.format = source_layout(im, o, up)
            a.w, a.h = im.shape[1], im.shape[0]
    else:
        arr = (ImagePlanar * n)()
        for a, im, o, up in zip(arr, images, orders, ups):
            if kind == "float":
                a.d_pixels, a.row_pitch, a.plane_pitch, fmt.dtype = source_layout_float(im, o, up)
            else:
                a.d_pixels, a.row_pitch, a.plane_pitch = source_layout_planar(im, o, up)
            a.num_chans, a.h, a.w = im.shape
    for a, out in zip(arr, outs or ()):
        a.d_out, a.out_cap = out.data_ptr(), out.numel()
    return arr, fmt


def _record_channels(kind, arr):
    """PNG channels of every record of _source_records(.., kind, ..)"""
    return [format_channels(a.format) if kind == "ex" else a.num_chans for a in arr]


def _rendition_records(renditions):
    arr = (_lib.Rendition * len(renditions))()
    for i, r in enumerate(renditions):
        if not isinstance(r, _lib.Rendition):
            raise ValueError("renditions: a list of fpng_amd.rendition() records")
        C.memmove(C.byref(arr, i * C.sizeof(_lib.Rendition)), C.byref(r), C.sizeof(_lib.Rendition))
    return arr


def _as_tensors(images):
    images = [images] if isinstance(images, (torch.Tensor, np.ndarray)) else list(images)
    return [torch.from_numpy(im) if isinstance(im, np.ndarray) else im for im in images]


def renditions_plan(images, renditions, kind="image", packed=False, **layout):
    """fpng_amd_renditions_plan: the validation of Encoder.submit_renditions() without a GPU -- raises FpngAmdError as that call would --
    and (scratch bytes, [offset of every rendition's tight rows in the scratch]).  images: tensors as for submit_renditions (CPU
    tensors work: only their addresses and strides are looked at); a rendition's d_out / out_cap are judged as they stand in the
    record (packed=True: they must be unset)."""
    images = _as_tensors(images)
    arr, fmt = _source_records("renditions_plan", images, kind, **layout)
    rarr = _rendition_records(renditions)
    total, offs = C.c_uint64(0), (C.c_uint64 * len(rarr))()
    check(_lib.load().fpng_amd_renditions_plan(_DESC_KINDS[kind], C.cast(arr, C.c_void_p), len(arr), C.byref(fmt) if fmt is not None else None, rarr, len(rarr),
                                               1 if packed else 0, C.byref(total), offs))
    return total.value, list(offs)


def rendition_pixels(images, rendition, kind="image", **layout):
    """fpng_amd_rendition_pixels, the resize stage's host twin (no GPU; the text the kernel compiles): the (h, w, c) uint8 array of
    R,G,B[,A] pixels whose file Encoder.submit_renditions() writes for this record.  images: CPU tensors or numpy arrays in the
    layout of `kind` (one, or a list that the record's `image` indexes), with that kind's layout arguments."""
    images = _as_tensors(images)
    if any(im.is_cuda for im in images):
        raise ValueError("rendition_pixels: host tensors (the twin runs on the CPU)")
    arr, fmt = _source_records("rendition_pixels", images, kind, **layout)
    c = _record_channels(kind, arr)[rendition.image] if rendition.image < len(arr) else 4
    out = np.empty((max(rendition.h, 1), max(rendition.w, 1), c), dtype=np.uint8)
    check(_lib.load().fpng_amd_rendition_pixels(_DESC_KINDS[kind], C.cast(arr, C.c_void_p), len(arr), C.byref(fmt) if fmt is not None else None, C.byref(rendition),
                                                out.ctypes.data, out.size))
    return out


# ---- YUV video frames: encoding straight from a decoder's surfaces (fpng_amd_encode_submit_yuv) ----
YUV_SURFACES = _lib.YUV_SURFACES    # name -> FPNG_AMD_YUV_*: "nv12", "p016" (also P010 / P012), "yuv444", "yuv444_16"
YUV_STANDARDS = _lib.YUV_STANDARDS  # name -> FPNG_AMD_YUV_BT*: "bt601", "bt709", "bt2020"


def yuv_matrix(standard="bt709", full_range=False):
    """fpng_amd_yuv_matrix: the (3, 4) float32 matrix [R, G, B] = m[:, :3] @ [Y, Cb, Cr] + m[:, 3] of "bt601", "bt709" or "bt2020",
    limited (Y 16..235, C 16..240) or full range, for 8-bit values -- 16-bit elements count as word / 256, so the same matrix
    serves P010 / P012 / P016.  Swap columns 1 and 2 for NV21 / YVU orders."""
    if standard not in YUV_STANDARDS:
        raise ValueError(f"yuv_matrix: standard {standard!r} ({', '.join(sorted(YUV_STANDARDS))})")
    m = np.empty((3, 4), dtype=np.float32)
    check(_lib.load().fpng_amd_yuv_matrix(YUV_STANDARDS[standard], 1 if full_range else 0, m.ctypes.data_as(C.POINTER(C.c_float))))
    return m


def _yuv_format(who, surface, matrix, standard, full_range):
    if surface not in YUV_SURFACES:
        raise ValueError(f"{who}: surface {surface!r} ({', '.join(sorted(YUV_SURFACES))})")
    m = yuv_matrix(standard, full_range) if matrix is None else np.asarray(matrix, dtype=np.float32)
    if m.shape != (3, 4):
        raise ValueError(f"{who}: matrix is 3 x 4, not {m.shape}")
    fmt = _lib.YuvFormat()
    fmt.surface = YUV_SURFACES[surface]
    for c in range(3):
        for k in range(4):
            fmt.m[c][k] = float(m[c, k])
    return fmt


def yuv_frame_layout(frame, surface="nv12"):
    """(d_luma, row_pitch, chroma_offset, w, h) of an fpng_amd_yuv_frame for a tuple of tensor views of ONE surface, from data_ptr()
    and strides alone: (Y (h, w), CbCr (ceil(h / 2), ceil(w / 2), 2)) for "nv12" / "p016", (Y, Cb, Cr), each (h, w), for "yuv444" /
    "yuv444_16"; uint8, or uint16 / int16 for the 16-bit surfaces.  ValueError when the planes' row strides differ, when elements
    are not tight, or when (4:4:4) Cr - Cb is not Cb - Y.  row_pitch 0 stands for tight rows where no plane has a second row."""
    who = "yuv_frame_layout"
    if surface not in YUV_SURFACES:
        raise ValueError(f"{who}: surface {surface!r} ({', '.join(sorted(YUV_SURFACES))})")
    s = YUV_SURFACES[surface]
    is420, elem = s < 2, 2 if s & 1 else 1
    planes = [torch.from_numpy(p) if isinstance(p, np.ndarray) else p for p in frame]
    if len(planes) != (2 if is420 else 3) or not all(isinstance(p, torch.Tensor) for p in planes):
        raise ValueError(f"{who}: a {surface} frame is a tuple of {'(Y, CbCr)' if is420 else '(Y, Cb, Cr)'} tensors")
    dtypes = (torch.uint8,) if elem == 1 else tuple(d for d in (getattr(torch, "uint16", None), torch.int16) if d is not None)
    if not all(p.dtype in dtypes for p in planes):
        raise ValueError(f"{who}: {surface} planes are {' or '.join(str(d) for d in dtypes)} tensors")
    y = planes[0]
    if y.dim() != 2 or not y.shape[0] or not y.shape[1]:
        raise ValueError(f"{who}: Y is shaped (h, w)")
    h, w = y.shape
    for p in planes[1:]:
        want = ((h + 1) // 2, (w + 1) // 2, 2) if is420 else (h, w)
        if tuple(p.shape) != want:
            raise ValueError(f"{who}: a chroma plane of a {w} x {h} {surface} frame is shaped {want}, not {tuple(p.shape)}")
    pitches = set()
    for p in planes:
        # (the stride of a dimension of one element says nothing)
        inner = [(p.shape[1], p.stride(1), p.shape[2] if p.dim() == 3 else 1)] + ([(2, p.stride(2), 1)] if p.dim() == 3 else [])
        if any(n > 1 and st != step for n, st, step in inner):
            raise ValueError(f"{who}: the elements of a row are not tight (strides {tuple(p.stride())})")
        if p.shape[0] > 1:
            pitches.add(p.stride(0) * elem)
    if len(pitches) > 1:
        raise ValueError(f"{who}: the planes' row strides differ ({sorted(pitches)} bytes): a surface has one pitch")
    offs = [p.data_ptr() - q.data_ptr() for p, q in zip(planes[1:], planes[:-1])]
    if len(set(offs)) > 1:
        raise ValueError(f"{who}: Cr - Cb ({offs[1]} bytes) is not Cb - Y ({offs[0]} bytes)")
    return y.data_ptr(), (pitches.pop() if pitches else 0), offs[0], w, h


def _yuv_records(who, frames, surface, outs=None):
    frames = [tuple(f) for f in frames]
    if outs is not None and len(outs) != len(frames):
        raise ValueError(f"{who}: {len(frames)} frames, {len(outs)} outs")
    arr = (_lib.YuvFrame * len(frames))()
    for a, f in zip(arr, frames):
        a.d_luma, a.row_pitch, a.chroma_offset, a.w, a.h = yuv_frame_layout(f, surface)
    for a, out in zip(arr, outs or ()):
        a.d_out, a.out_cap = out.data_ptr(), out.numel()
    return frames, arr


def yuv_pixels(frames, surface="nv12", matrix=None, standard="bt709", full_range=False, frame=0, rendition=None):
    """fpng_amd_yuv_pixels, the conversion's host twin (no GPU; the text the kernels compile): the (h, w, 3) uint8 array of R,G,B
    pixels whose file Encoder.submit_yuv() writes for frame `frame` of `frames` (CPU tensors or numpy arrays, each a tuple as for
    yuv_frame_layout) -- or, with an fpng_amd.rendition() record, for that rendition of it (the record's `image` is not looked at)."""
    frames, arr = _yuv_records("yuv_pixels", frames, surface)
    if any(p.is_cuda for f in frames for p in f if isinstance(p, torch.Tensor)):
        raise ValueError("yuv_pixels: host tensors (the twin runs on the CPU)")
    fmt = _yuv_format("yuv_pixels", surface, matrix, standard, full_range)
    if rendition is not None:
        shape = (max(rendition.h, 1), max(rendition.w, 1), 3)
    else:
        shape = (arr[frame].h, arr[frame].w, 3) if 0 <= frame < len(arr) else (1, 1, 3)
    out = np.empty(shape, dtype=np.uint8)
    check(_lib.load().fpng_amd_yuv_pixels(arr, len(arr), C.byref(fmt), _u32("yuv_pixels", "frame", frame), C.byref(rendition) if rendition is not None else None,
                                          out.ctypes.data, out.size))
    return out


class _NoOut:
    """stands in a make_batch_packed() descriptor where the other makers' hold an output tensor: a packed submission has none"""
    is_cuda = True


def _need_cuda(who, tensors, what):
    if not all(isinstance(t, torch.Tensor) and t.is_cuda for t in tensors):
        raise ValueError(f"{who}: {what} are CUDA tensors")


def _own_batch(who, maker, batch, record, size=3):
    """the prebuilt descriptor of a submit call is its own maker's: anything else is refused before the library is touched"""
    if not (isinstance(batch, tuple) and len(batch) == size and isinstance(batch[2], C.Array) and batch[2]._type_ is record):
        raise ValueError(f"{who}: without outs, images is a {maker}() descriptor")
    return batch


def _pack_record(who, arena, align, lead, table, n):
    """the fpng_amd_pack of a packed call of n files: its arena and, if given, its table, checked"""
    if not (isinstance(arena, torch.Tensor) and arena.is_cuda and arena.dtype == torch.uint8 and arena.is_contiguous()):
        raise ValueError(f"{who}: arena is a contiguous uint8 CUDA tensor")
    pack = _lib.Pack(arena.data_ptr(), arena.numel(), align, lead, None, 0)
    if table is not None:
        if not (table.is_cuda and table.dtype == torch.int64 and table.is_contiguous() and table.numel() >= 2 * (n + 1)):
            raise ValueError(f"{who}: table is a contiguous int64 CUDA tensor of 2 * (n + 1) elements")
        pack.d_table = table.data_ptr()
    return pack


def _files(outs, records):
    """the files of a finished submission as bytes: outs[i][:png_size], or FpngAmdError for the first record with a status"""
    pngs = []
    for out, (size, _, status) in zip(outs, records):
        if status:
            raise FpngAmdError(status, "device reported an encode failure")
        pngs.append(bytes(out[:size].cpu().numpy()))
    return pngs


def layout_1pass(num_chans):
    a, b, c = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    check(_lib.load().fpng_amd_1pass_layout(num_chans, C.byref(a), C.byref(b), C.byref(c)))
    return a.value, b.value, c.value


HW_QUEUE_SOURCES = ("library_set", "caller_set", "driver_open", "hands_off")  # FPNG_AMD_HWQ_* (include/fpng_amd.h)


def runtime_info():
    """fpng_amd_runtime_info(): {"hw_queues", "hw_queue_source", "lanes"} -- the hardware queues the library believes the HIP runtime
    uses, why (it asks for eight when it is loaded before the process's first HIP call), and the lanes a new encoder would get."""
    info = _lib.RuntimeInfo()
    check(_lib.load().fpng_amd_runtime_info(C.byref(info)))
    return {"hw_queues": int(info.hw_queues), "hw_queue_source": HW_QUEUE_SOURCES[info.hw_queue_source], "lanes": int(info.lanes)}


def release_cached_memory():
    """Free the device buffers that destroyed encoders left with the library (fpng_amd_release_cached_memory)."""
    check(_lib.load().fpng_amd_release_cached_memory())


def pin_host_memory(arr):
    """Page-lock a numpy array's memory (fpng_amd_pin_host_memory): saves the runtime's pinning of every chunk it copies.
    Unpin before the array is freed."""
    check(_lib.load().fpng_amd_pin_host_memory(arr.ctypes.data, arr.nbytes))


def unpin_host_memory(arr):
    check(_lib.load().fpng_amd_unpin_host_memory(arr.ctypes.data))


def plan_bands(stats, w, h, num_chans, flags=0):
    """fpng_amd_plan_bands: stats = list of _lib.BandStats in row order -> (start_bits, BandPlan)."""
    n = len(stats)
    arr = (_lib.BandStats * n)(*stats)
    starts = (C.c_uint64 * n)()
    plan = _lib.BandPlan()
    check(_lib.load().fpng_amd_plan_bands(arr, n, w, h, num_chans, flags, starts, C.byref(plan)))
    return list(starts), plan


def band_window(is_first, is_last, start_bit, token_bits, eob_bits):
    """-> (file offset, bytes, shared head bytes) of the window fpng_amd_band_place() writes."""
    off, n, hd = C.c_uint64(0), C.c_size_t(0), C.c_uint32(0)
    check(_lib.load().fpng_amd_band_window(int(is_first), int(is_last), start_bit, token_bits, eob_bits, C.byref(off), C.byref(n), C.byref(hd)))
    return off.value, n.value, hd.value


def idat_crc_from_bands(raw, ends, zlib_size, adler):
    n = len(raw)
    return _lib.load().fpng_amd_idat_crc_from_bands((C.c_uint32 * n)(*raw), (C.c_uint64 * n)(*ends), n, zlib_size, adler)


def png_head(w, h, num_chans, zlib_size):
    b = (C.c_uint8 * 58)()
    check(_lib.load().fpng_amd_png_head(w, h, num_chans, zlib_size, b))
    return bytes(b)


def png_tail(adler, idat_crc):
    b = (C.c_uint8 * 20)()
    _lib.load().fpng_amd_png_tail(adler, idat_crc, b)
    return bytes(b)


class Node:
    """fpng_amd_node: one process, one encoder + staging ring per listed device, host batches dealt round-robin."""

    def __init__(self, devices):
        self.lib = _lib.load()
        h = C.c_void_p()
        arr = (C.c_int * len(devices))(*devices)
        check(self.lib.fpng_amd_node_create(C.byref(h), arr, len(devices)))
        self.h = h

    def size(self):
        return self.lib.fpng_amd_node_size(self.h)

    def encode_host_batch(self, images, flags=0, outs=None, paths=None, writer_threads=0):
        arr, sizes, keep = _host_batch_records(images, outs, paths)
        check(self.lib.fpng_amd_node_encode_host_batch(self.h, arr, len(images), flags, writer_threads))
        return [int(s) for s in sizes]

    def encode_host_image(self, image, w, h, num_chans, flags=0, out=None):
        """fpng_amd_node_encode_host_image: ONE host image (uint8 array) cut into row bands over the node's devices.  out=None ->
        the PNG as bytes (byte-identical to the single-device encoders' and to the reference's); out = a uint8 numpy array of at
        least max_encoded_size() bytes -> the file is written into it and its size returned (no allocation: a capture loop's form)."""
        b = _as_u8(image)
        if b.size < w * h * num_chans:
            raise ValueError("image buffer smaller than w*h*num_chans")
        buf = out if out is not None else np.empty(max_encoded_size(w, h, num_chans), dtype=np.uint8)
        assert buf.dtype == np.uint8 and buf.flags["C_CONTIGUOUS"]

        def reserve(_user, nbytes):  # (one buffer that only ever "grows" inside its capacity: what was written stays)
            return buf.ctypes.data if nbytes <= buf.size else None

        cb = _lib.RESERVE_FN(reserve)
        n = C.c_size_t(0)
        check(self.lib.fpng_amd_node_encode_host_image(self.h, b.ctypes.data, w, h, num_chans, flags, cb, None, C.byref(n)))
        return n.value if out is not None else buf[: n.value].tobytes()

    def close(self):
        if getattr(self, "h", None):
            self.lib.fpng_amd_node_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _host_batch_records(images, outs, paths):
    n = len(images)
    arr = (HostImage * n)()
    sizes = (C.c_size_t * n)()
    keep = []
    for i, im in enumerate(images):
        im = np.ascontiguousarray(im, dtype=np.uint8)
        keep.append(im)
        h, w, c = im.shape
        arr[i].pixels = im.ctypes.data
        arr[i].w, arr[i].h, arr[i].num_chans = w, h, c
        if outs is not None:
            arr[i].out = outs[i].ctypes.data
            arr[i].out_cap = outs[i].size
        arr[i].out_size = C.cast(C.byref(sizes, i * C.sizeof(C.c_size_t)), C.POINTER(C.c_size_t))
        if paths is not None:
            p = paths[i].encode() if isinstance(paths[i], str) else paths[i]
            keep.append(p)
            arr[i].path = p
    return arr, sizes, keep


def synth_image(kind, w, h, num_chans, seed=12345):
    """Deterministic test image as a uint8 array of shape (h, w, num_chans)."""
    out = np.empty(w * h * num_chans, dtype=np.uint8)
    check(_lib.load().fpng_amd_synth_image(SYNTH_KINDS[kind], seed, w, h, num_chans, out.ctypes.data))
    return out.reshape(h, w, num_chans)


# The views calls' stages in the order the C calls take their record arrays: (keyword, the descriptor's attribute, the record's
# class, what to say of an entry that is no such record where the keyword has a wording of its own).  The last stage whose records a
# descriptor carries names the call.  color and resample take more than records: _color_records / _resample_arg convert them.
_VIEW_STAGES = (("color", "colors", _lib.ViewColor, None),
                ("post", "posts", _lib.ViewPost, "a post record is what view_post() returns"),
                ("warp", "warps", _lib.ViewWarp, "a warp record is what view_warp() returns"),
                ("tone", "tones", _lib.ViewTone, None),
                ("enhance", "enhances", _lib.ViewEnhance, None),
                ("alpha", "alphas", _lib.ViewAlpha, None),
                ("resample", "resamples", _lib.ViewResample, None))


class DecodeBatch:
    """What Encoder.make_decode_batch() returns: the files, the output tensors and the C arrays of one fpng_amd_decode_batch_device() call."""

    maker = "make_decode_batch"

    def __init__(self, pngs, outs, arr, res, desired_chans):
        self.pngs, self.outs, self.arr, self.res, self.desired_chans = pngs, outs, arr, res, desired_chans

    def statuses(self):
        """status of every file after the last call (one numpy view of the result records, no loop over them)"""
        return np.frombuffer(self.res, dtype=np.int32).reshape(-1, 4)[:, 3]

    def results(self):
        """list of (status, uint8 CUDA tensor (h, w, desired_chans) or None, channels_in_file)"""
        out, d = [], self.desired_chans
        for r, t in zip(self.res, self.outs):
            out.append((r.status, t.view(-1)[: r.w * r.h * d].view(r.h, r.w, d) if r.status == 0 else None, r.channels_in_file))
        return out


class _DecodeBatchViews:
    """The files, the caller's destination views and the C arrays of one decode call into views (DecodeBatchEx, DecodeBatchPlanar,
    DecodeBatchFloat, DecodeBatchCrop, DecodeBatchResize, DecodeBatchResizeView, DecodeBatchMultiView, DecodeBatchMultiViewHwc,
    DecodeBatchYuv).
    maker: the Encoder method that makes the class's descriptors; extras: the call's further arrays, stored under their names."""

    maker = None

    def __init__(self, pngs, outs, arr, res, device_data, keep, **extras):
        self.pngs, self.outs, self.arr, self.res, self.device_data, self._keep = pngs, outs, arr, res, device_data, keep
        self.__dict__.update(extras)

    @classmethod
    def call(cls, device_data):
        """the name of the Encoder method that runs the class's descriptors of files in device / host memory"""
        return ("decode_device" if device_data else "decode_batch") + cls.maker[len("make_decode_batch"):]

    def tensors(self):
        """every destination view"""
        return self.outs

    def statuses(self):
        """status of every file after the last call"""
        return np.frombuffer(self.res, dtype=np.int32).reshape(-1, 4)[:, 3]

    def results(self):
        """list of (status, the caller's own destination view (filled in place) or None, channels_in_file)"""
        return [(r.status, t if r.status == 0 else None, r.channels_in_file) for r, t in zip(self.res, self.outs)]


class DecodeBatchEx(_DecodeBatchViews):
    """What Encoder.make_decode_batch_ex() returns: the files, the caller's destination views and the C arrays of one
    fpng_amd_decode_batch(_device)_ex() call."""

    maker = "make_decode_batch_ex"


class DecodeBatchPng(_DecodeBatchViews):
    """What Encoder.make_decode_batch_png() returns: the files (ordinary PNGs), the output tensors and the C arrays of one
    fpng_amd_decode_batch(_device)_png() call."""

    maker = "make_decode_batch_png"

    def results(self):
        """list of (status, uint8 CUDA tensor (h, w, desired_chans) or None, channels_in_file)"""
        out, d = [], self.desired_chans
        for r, t in zip(self.res, self.outs):
            out.append((r.status, t.view(-1)[: r.w * r.h * d].view(r.h, r.w, d) if r.status == 0 else None, r.channels_in_file))
        return out


class DecodeBatchPlanar(_DecodeBatchViews):
    """What Encoder.make_decode_batch_planar() returns: the same for one fpng_amd_decode_batch(_device)_planar() call (outs: the
    caller's (c, h, w) views).  Not a DecodeBatchEx: neither call takes the other's descriptor."""

    maker = "make_decode_batch_planar"


class DecodeBatchFloat(_DecodeBatchViews):
    """What Encoder.make_decode_batch_float() returns: the same for one fpng_amd_decode_batch(_device)_planar_float() call (outs: the
    caller's float (c, h, w) views, all of one dtype; fmt: the call's fpng_amd_float_format).  Neither a DecodeBatchPlanar nor a
    DecodeBatchEx: no call takes another's descriptor."""

    maker = "make_decode_batch_float"


class DecodeBatchCrop(_DecodeBatchViews):
    """What Encoder.make_decode_batch_crop() returns: the same for one fpng_amd_decode_batch(_device)_planar_crop() call (crops: the
    fpng_amd_crop[n]; outs: the caller's (c, crop h, crop w) views, uint8 or all of one float dtype; fmt: the call's
    fpng_amd_float_format, None for uint8 planes).  No other call takes this descriptor."""

    maker = "make_decode_batch_crop"


class DecodeBatchResize(_DecodeBatchViews):
    """What Encoder.make_decode_batch_resize() returns: the same for one fpng_amd_decode_batch(_device)_planar_resize() call (crops:
    the fpng_amd_crop[n]; sizes: the fpng_amd_resize[n]; outs: the caller's (c, out_h, out_w) views, uint8 or all of one float
    dtype; fmt: the call's fpng_amd_float_format, None for uint8 planes).  No other call takes this descriptor."""

    maker = "make_decode_batch_resize"


class DecodeBatchResizeView(_DecodeBatchViews):
    """What Encoder.make_decode_batch_resize_view() returns: the same for one fpng_amd_decode_batch(_device)_planar_resize_view() call
    (crops: the fpng_amd_crop[n]; views: the fpng_amd_resize_view[n]; outs: the caller's (c, window h, window w) views, uint8 or all
    of one float dtype; fmt: the call's fpng_amd_float_format, None for uint8 planes).  No other call takes this descriptor."""

    maker = "make_decode_batch_resize_view"


class _DecodeBatchMultiViews(_DecodeBatchViews):
    """What the descriptors of the views calls share, whatever the destinations' layout.  colors, posts, warps, tones, enhances,
    alphas, resamples (_VIEW_STAGES): the records, one per view, of a descriptor made with color=, post=, ..., else None; the call is
    then the _views_color, _views_post, ... one."""

    def __init__(self, pngs, outs, arr, res, device_data, keep, counts, crops, views, dests, fmt):
        super().__init__(pngs, outs, arr, res, device_data, keep, counts=counts, crops=crops, views=views, dests=dests, fmt=fmt)
        for _, attr, _, _ in _VIEW_STAGES:
            setattr(self, attr, None)

    def tensors(self):
        return [t for ts in self.outs for t in ts]

    def results(self):
        """list, per file, of (status, the list of the caller's own destination views (filled in place) or None, channels_in_file)"""
        return [(r.status, list(ts) if r.status == 0 else None, r.channels_in_file) for r, ts in zip(self.res, self.outs)]


class DecodeBatchMultiView(_DecodeBatchMultiViews):
    """What Encoder.make_decode_batch_views() returns: the same for one fpng_amd_decode_batch(_device)_planar_views() call, which
    writes SEVERAL views of each file (counts: the uint32[n] views per file; crops, views, dests: the fpng_amd_crop,
    fpng_amd_resize_view and fpng_amd_view_dest records, one per view, file 0's first; outs: per file the list of the caller's (c,
    window h, window w) views, uint8 or all of one float dtype; fmt: the call's fpng_amd_float_format, None for uint8 planes).  No
    other call takes this descriptor.  colors: the fpng_amd_view_color records of a descriptor made with color=, one per view (the
    call is then fpng_amd_decode_batch(_device)_planar_views_color), else None."""

    maker = "make_decode_batch_views"


class DecodeBatchMultiViewHwc(_DecodeBatchMultiViews):
    """What Encoder.make_decode_batch_views_hwc() returns: DecodeBatchMultiView's twin for one
    fpng_amd_decode_batch(_device)_hwc_views() call (dests: the fpng_amd_view_dest_hwc records; outs: per file the list of the
    caller's (window h, window w, c) views; colors: as DecodeBatchMultiView's, for fpng_amd_decode_batch(_device)_hwc_views_color).
    No other call takes this descriptor."""

    maker = "make_decode_batch_views_hwc"


class DecodeBatchPngViews(_DecodeBatchMultiViews):
    """What Encoder.make_decode_batch_png_views() returns for layout="planar": DecodeBatchMultiView's descriptor for ORDINARY PNG
    files and one fpng_amd_decode_batch(_device)_png_views() call (flags: the call's, FPNG_AMD_PNG_GENERAL_ONLY).  No other call
    takes this descriptor."""

    maker = "make_decode_batch_png_views"
    flags = 0


class DecodeBatchPngViewsHwc(DecodeBatchPngViews):
    """... and for layout="hwc": DecodeBatchMultiViewHwc's twin (dests: the fpng_amd_view_dest_hwc records)."""


def _planar_view_dest(rec, t, order, bottom_up, is_u8):
    """the fpng_amd_view_dest of a (c, h, w) view; -> the float format's dtype code, or None"""
    if is_u8:
        (ptr, rp, pp), code = dest_layout_planar(t, order, bottom_up), None
    else:
        ptr, rp, pp, code = dest_layout_float(t, order, bottom_up)
    c, oh, ow = t.shape
    rec.d_pixels, rec.row_pitch, rec.plane_pitch = ptr, rp, pp
    rec.pixels_cap = (c - 1) * abs(pp) + (oh - 1) * abs(rp) + ow * t.element_size()  # (the view's own spans, in bytes)
    return code


def _hwc_view_dest(rec, t, order, bottom_up, is_u8):
    """the fpng_amd_view_dest_hwc of an (h, w, c) view; -> the float format's dtype code, or None"""
    ptr, rp, px, flags, code = dest_layout_hwc(t, order, bottom_up)
    oh, ow, c = t.shape
    rec.d_pixels, rec.row_pitch, rec.pixel_elems, rec.flags = ptr, rp, px, flags
    rec.pixels_cap = (oh - 1) * abs(rp) + ((ow - 1) * px + c) * t.element_size()  # (the view's own spans, in bytes)
    return code


class _ViewsLayout:
    """What the views calls' two destination layouts differ in.  name: the layout's part of the C symbols; dest_cls, batch_cls: the
    destination record and the descriptor, whose maker names the Python methods; put_dest: writes a tensor view's destination record
    (its layout function and pixels_cap formula); chw: a view's shape as (c, h, w); empty_shape: of an allocated (oh, ow) output."""

    def __init__(self, name, dest_cls, batch_cls, put_dest, chw, empty_shape, fmt=None):
        self.name, self.dest_cls, self.batch_cls, self.put_dest, self.chw, self.empty_shape = name, dest_cls, batch_cls, put_dest, chw, empty_shape
        self.fmt = fmt  # the call's own format record in the place of the float format (the YUV layout's), else None
        self.maker, self.host, self.device = batch_cls.maker, batch_cls.call(False), batch_cls.call(True)


class DecodeBatchYuv(_DecodeBatchMultiViews):
    """What Encoder.make_decode_batch_yuv() returns: DecodeBatchMultiView's twin for one fpng_amd_decode_batch(_device)_yuv_views()
    call (dests: the fpng_amd_yuv_dest records; outs: per file the list of the caller's surfaces, each a YuvSurface -- the tuple of
    plane tensors yuv_frame_layout() takes; fmt: the call's fpng_amd_yuv_store_format).  No other call takes this descriptor."""

    maker = "make_decode_batch_yuv"


class YuvSurface(tuple):
    """a YUV surface as a destination of the views machinery: the tuple of its plane tensors (yuv_frame_layout() has the shapes),
    which answers the questions that machinery asks a destination tensor"""

    @property
    def shape(self):
        return (3,) + tuple(self[0].shape)

    @property
    def is_cuda(self):
        return all(p.is_cuda for p in self)


def yuv_surface_bytes(surface, w, h, row_pitch, chroma_offset):
    """fpng_amd_yuv_dest::surface_cap of a w x h surface with these layout words: the bytes from the top row of its lowest-addressed
    plane to the last element of its highest one"""
    s = YUV_SURFACES[surface]
    elem = 2 if s & 1 else 1
    chroma_row = (2 * ((w + 1) // 2) if s < 2 else w) * elem
    pitch = row_pitch or max(w * elem, chroma_row)
    span = (h - 1) * pitch + w * elem
    if s >= 2:
        return 2 * abs(chroma_offset) + span
    return abs(chroma_offset) + (span if chroma_offset < 0 else ((h + 1) // 2 - 1) * pitch + chroma_row)


def _yuv_views(surface, fmt):
    """the views calls' layout (_ViewsLayout) whose destinations are surfaces of `surface` under the call's format `fmt`"""

    def put_dest(rec, t, order, bottom_up, is_u8):
        rec.d_luma, rec.row_pitch, rec.chroma_offset, w, h = yuv_frame_layout(t, surface)
        rec.surface_cap = yuv_surface_bytes(surface, w, h, rec.row_pitch, rec.chroma_offset)
        return None

    return _ViewsLayout("yuv", _lib.YuvDest, DecodeBatchYuv, put_dest, lambda s: (s[0], s[1], s[2]), None, fmt)


def _yuv_store_format(who, surface, depth, matrix, standard, full_range):
    if surface not in YUV_SURFACES:
        raise ValueError(f"{who}: surface {surface!r} ({', '.join(sorted(YUV_SURFACES))})")
    m = yuv_matrix_from_rgb(standard, full_range) if matrix is None else np.asarray(matrix, dtype=np.float32)
    if m.shape != (3, 4):
        raise ValueError(f"{who}: matrix is 3 x 4, not {m.shape}")
    fmt = _lib.YuvStoreFormat()
    fmt.surface, fmt.depth = YUV_SURFACES[surface], _u32(who, "depth", depth or 0)
    for c in range(3):
        for k in range(4):
            fmt.m[c][k] = float(m[c, k])
    return fmt


def yuv_matrix_from_rgb(standard="bt709", full_range=False):
    """fpng_amd_yuv_matrix_from_rgb: the (3, 4) float32 matrix [Y, Cb, Cr] = m[:, :3] @ [R, G, B] + m[:, 3] of "bt601", "bt709" or
    "bt2020", limited (Y 16..235, C 16..240) or full range, in 8-bit units -- the decode side's direction, the other way round from
    yuv_matrix().  Swap rows 1 and 2 for NV21 / YVU orders."""
    if standard not in YUV_STANDARDS:
        raise ValueError(f"yuv_matrix_from_rgb: standard {standard!r} ({', '.join(sorted(YUV_STANDARDS))})")
    m = np.empty((3, 4), dtype=np.float32)
    check(_lib.load().fpng_amd_yuv_matrix_from_rgb(YUV_STANDARDS[standard], 1 if full_range else 0, m.ctypes.data_as(C.POINTER(C.c_float))))
    return m


def yuv_surface_planes(surface, w, h, make):
    """the planes of a tight w x h surface as views of ONE buffer: make(n, elem_bytes) returns a flat array or tensor of n elements of
    that size, which has reshape and basic slicing -> the tuple yuv_frame_layout() takes"""
    s = YUV_SURFACES[surface]
    elem = 2 if s & 1 else 1
    if s >= 2:
        buf = make(3 * h * w, elem).reshape(3, h, w)
        return (buf[0], buf[1], buf[2])
    cw, ch = (w + 1) // 2, (h + 1) // 2
    rows = make((h + ch) * 2 * cw, elem).reshape(h + ch, 2 * cw)
    return (rows[:h, :w], rows[h:].reshape(ch, cw, 2))


def yuv_surface(rgb, surface="nv12", depth=None, matrix=None, standard="bt709", full_range=False):
    """fpng_amd_yuv_surface, the host twin of Encoder.decode_device_yuv()'s last stage (no GPU; the text the kernel compiles): the
    planes of the tight surface -- numpy arrays, as yuv_frame_layout() takes them -- for the (h, w, 3) uint8 array of R,G,B pixels
    `rgb`.  depth: None (the surface's own: 8 / 16), or 10, 12 or 16 on the 16-bit surfaces; matrix: a (3, 4) matrix of the
    caller's, else yuv_matrix_from_rgb(standard, full_range)."""
    who = "yuv_surface"
    rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
    if rgb.ndim != 3 or rgb.shape[2] != 3 or not rgb.shape[0] or not rgb.shape[1]:
        raise ValueError(f"{who}: rgb is an (h, w, 3) uint8 array")
    fmt = _yuv_store_format(who, surface, depth, matrix, standard, full_range)
    h, w = rgb.shape[:2]
    planes = yuv_surface_planes(surface, w, h, lambda n, elem: np.zeros(n, dtype=np.uint8 if elem == 1 else np.uint16))
    rec = _lib.YuvDest()
    rec.d_luma, rec.row_pitch, rec.chroma_offset, _, _ = yuv_frame_layout(planes, surface)
    rec.surface_cap = yuv_surface_bytes(surface, w, h, rec.row_pitch, rec.chroma_offset)
    check(_lib.load().fpng_amd_yuv_surface(rgb.ctypes.data, w, h, C.byref(fmt), C.byref(rec)))
    return planes


def _png_size(png):
    """(w, h) of a file from its IHDR, for the calls that take the whole file at its own size by default (a device file: 8 bytes come back)"""
    head = bytes(png[16:24].cpu().numpy()) if isinstance(png, torch.Tensor) else bytes(png)[16:24]
    if len(head) != 8:
        raise ValueError("a file of fewer than 24 bytes has no size")
    return int.from_bytes(head[:4], "big"), int.from_bytes(head[4:], "big")


_PLANAR_VIEWS = _ViewsLayout("planar", _lib.ViewDest, DecodeBatchMultiView, _planar_view_dest, lambda s: (s[0], s[1], s[2]), lambda oh, ow: (3, oh, ow))
_HWC_VIEWS = _ViewsLayout("hwc", _lib.ViewDestHwc, DecodeBatchMultiViewHwc, _hwc_view_dest, lambda s: (s[2], s[0], s[1]), lambda oh, ow: (oh, ow, 3))


_PNG_VIEWS = {"planar": _ViewsLayout("planar", _lib.ViewDest, DecodeBatchPngViews, _planar_view_dest, _PLANAR_VIEWS.chw, _PLANAR_VIEWS.empty_shape),
              "hwc": _ViewsLayout("hwc", _lib.ViewDestHwc, DecodeBatchPngViewsHwc, _hwc_view_dest, _HWC_VIEWS.chw, _HWC_VIEWS.empty_shape)}


def _per_file(who, n, v, what):
    """an argument of a per-file call -> a list with a value per file.  v: one value (_VIEW_ARG has what one looks like) for all
    files, or a sequence with one per file"""
    vs = [v] * n if _VIEW_ARG[what](v) else list(v)
    if len(vs) != n:
        raise ValueError(f"{who}: {n} files, {len(vs)} {what}")
    return vs


def _file_records(who, pngs, arr):
    """data and size of the file records arr[len(pngs)] of any decode call into views: uint8 CUDA tensors holding whole files, or
    bytes-like objects in host memory, one kind per call.  -> (device_data, keep: the host copies the records point into)"""
    device_data = len(pngs) > 0 and isinstance(pngs[0], torch.Tensor) and pngs[0].is_cuda
    keep = []
    for i, p in enumerate(pngs):
        if device_data:
            if not (isinstance(p, torch.Tensor) and p.is_cuda and p.dtype == torch.uint8 and p.is_contiguous()):
                raise ValueError(f"{who}: device files are contiguous uint8 CUDA tensors, all of them")
            arr[i].data, arr[i].size = (p.data_ptr() if p.numel() else None), p.numel()
        else:
            b = np.frombuffer(bytes(p), dtype=np.uint8)
            keep.append(b)
            arr[i].data, arr[i].size = (b.ctypes.data if b.size else None), b.size
    return device_data, keep


def _dest_format(who, outs, mean, std, scale, bias, always=False):
    """The destinations of one call (outs: all of them, in one list) share one dtype: -> (is_u8, the call's fpng_amd_float_format
    from its constants -- None for uint8 destinations, which take no constants).  always: the call has a format whatever the dtype
    (make_decode_batch_float, whose layout function refuses the uint8 views).  The format's dtype is the views' to fill in."""
    dtypes = {t.dtype for t in outs if isinstance(t, torch.Tensor)}
    if len(dtypes) > 1:
        raise ValueError(f"{who}: the destinations of one call share one dtype, not {sorted(str(d) for d in dtypes)}")
    is_u8 = dtypes == {torch.uint8}
    if is_u8 and not always:
        if any(v is not None for v in (mean, std, scale, bias)):
            raise ValueError(f"{who}: mean / std / scale / bias go with float destinations, not uint8 ones")
        return True, None
    sc, bi = _float_constants(who, normalize_constants, mean, std, scale, bias)
    fmt = _lib.FloatFormat()
    for k in range(4):
        fmt.scale[k], fmt.bias[k] = float(sc[k]), float(bi[k])
    return is_u8, fmt


def _planar_dests(arr, outs, orders, ups, is_u8, fmt):
    """the destination part of a per-file call's fpng_amd_png_planar records: file i's is its (c, h, w) view outs[i], as the views
    calls describe one (_planar_view_dest); float views put their dtype into fmt"""
    for rec, t, order, up in zip(arr, outs, orders, ups):
        code = _planar_view_dest(rec, t, order, up, is_u8)
        rec.num_chans = t.shape[0]
        if code is not None:
            fmt.dtype = code


def _window_hw(full, window):
    """(h, w) of the window (x, y, w, h) -- None: the whole -- of an image resized to full = (full_w, full_h)"""
    return (int(window[3]), int(window[2])) if window is not None else (int(full[1]), int(full[0]))


def _alloc_dtype(who, dtype):
    """the dtype= of a call that allocates its destinations"""
    if dtype is not torch.uint8 and dtype not in FLOAT_DTYPES:
        raise ValueError(f"{who}: dtype {dtype} (torch.uint8, float32, float16 or bfloat16)")
    return dtype


def _fmt_ref(batch):
    return C.byref(batch.fmt) if batch.fmt is not None else None


def _file_symbol(stem, device_data):
    """the C entry point of a per-file decode call into views: fpng_amd_decode_batch(_device)_<stem>"""
    return f"fpng_amd_decode_batch{'_device' if device_data else ''}_{stem}"


def _make_views_batch(layout, pngs, crops, outs, full, window, filter, mirror, order, bottom_up, mean, std, scale, bias, stages):
    """the descriptor of a views call for either layout (Encoder.make_decode_batch_views / _hwc have the rules).  stages: the stage
    keywords' values by keyword (_VIEW_STAGES)"""
    who = layout.maker
    n = len(pngs)
    if len(crops) != n or len(outs) != n:
        raise ValueError(f"{who}: {n} files, {len(crops)} lists of crops, {len(outs)} lists of destinations")
    crops, outs = [list(c) for c in crops], [list(o) for o in outs]
    counts = [len(c) for c in crops]
    for i in range(n):
        if counts[i] < 1 or len(outs[i]) != counts[i]:
            raise ValueError(f"{who}: file {i} has {counts[i]} crops (at least one) and {len(outs[i])} destinations")
    fulls, windows = _per_view(who, counts, full, "full sizes"), _per_view(who, counts, window, "windows")
    filters, mirrors = _per_view(who, counts, filter, "filters"), _per_view(who, counts, mirror, "mirror flags")
    is_u8, fmt = (True, layout.fmt) if layout.fmt is not None else _dest_format(who, [t for ts in outs for t in ts], mean, std, scale, bias)
    orders, ups = _per_view(who, counts, order, "plane orders"), _per_view(who, counts, bottom_up, "bottom_up flags")
    total = sum(counts)
    arr = (_lib.PngPlanarIn * n)()
    narr = (C.c_uint32 * n)(*counts)
    carr, varr, darr = (_lib.Crop * total)(), (_lib.ResizeView * total)(), (layout.dest_cls * total)()
    res = (_lib.DecodeResult * n)()
    device_data, keep = _file_records(who, pngs, arr)
    at = 0
    for i in range(n):
        codes = [layout.put_dest(darr[at + k], t, orders[i][k], bool(ups[i][k]), is_u8) for k, t in enumerate(outs[i])]
        chans = {layout.chw(t.shape)[0] for t in outs[i]}
        if len(chans) != 1:
            raise ValueError(f"{who}: the destinations of file {i} share one channel count, not {sorted(chans)}")
        arr[i].num_chans = chans.pop()  # (d_pixels, the pitches and pixels_cap stay NULL / 0: the destinations are the views')
        for k, t in enumerate(outs[i]):
            if codes[k] is not None:
                fmt.dtype = codes[k]
            _crop_record(f"{who}: file {i}", crops[i][k], carr[at])
            v = _view_record(who, fulls[i][k], windows[i][k], filters[i][k], bool(mirrors[i][k]), varr[at])
            _, oh, ow = layout.chw(t.shape)
            if (oh, ow) != (v.h, v.w) or oh < 1 or ow < 1:
                raise ValueError(f"{who}: destination {k} of file {i} is {ow} x {oh}, its window {v.w} x {v.h}")
            at += 1
    batch = layout.batch_cls(list(pngs), outs, arr, res, device_data, keep, narr, carr, varr, darr, fmt)
    for key, attr, cls, wrong in _VIEW_STAGES:
        arg = stages.get(key)
        if arg is None:
            continue
        if key == "color":
            setattr(batch, attr, _color_records(who, counts, arg))
        else:
            setattr(batch, attr, _view_records(who, counts, _resample_arg(arg) if key == "resample" else arg, cls, key, wrong))
    return batch


def views_entry(layout, device_data, batch):
    """The C entry point of a views call and its arguments behind the encoder, as a pure function of the layout ("planar" / "hwc"),
    where the files are and the descriptor: the last stage in the order colour < post < warp < tone < enhance < alpha < resample whose records the
    descriptor carries names the call, and the call takes the record arrays of all stages up to it (None for those not given)."""
    arrays = [getattr(batch, attr) for _, attr, _, _ in _VIEW_STAGES]
    stages = max((k + 1 for k, a in enumerate(arrays) if a is not None), default=0)
    return _lib.views_symbol(layout, device_data, stages), [batch.arr, len(batch.arr), batch.counts, batch.crops, batch.views, batch.dests, *arrays[:stages], _fmt_ref(batch), batch.res]


def png_views_entry(layout, device_data, batch, flags):
    """The C entry point of a PNG views call and its arguments behind the encoder, as a pure function of the layout ("planar" /
    "hwc"), where the files are, the descriptor and the call's flags: fpng_amd_decode_batch(_device)_png_views takes every family
    through one fpng_amd_png_views record -- the destinations in `dests` or in `hwc`, the stage arrays the descriptor carries (NULL
    for those not given; the last one given names the family the request is judged as)."""
    rq = _lib.PngViews()
    rq.view_count, rq.crops, rq.views = batch.counts, batch.crops, batch.views
    setattr(rq, "hwc" if layout == "hwc" else "dests", batch.dests)
    if batch.fmt is not None:
        rq.fmt = C.pointer(batch.fmt)
    for _, attr, _, _ in _VIEW_STAGES:
        if getattr(batch, attr) is not None:
            setattr(rq, attr, getattr(batch, attr))
    rq.flags, rq.reserved = int(flags), 0
    return _lib.png_views_symbol(device_data), [batch.arr, len(batch.arr), C.byref(rq), batch.res]


class Encoder:
    """Reusable device scratch + the HIP stream submissions are ordered against (one Encoder per thread).
    `stream="torch"` (default): every submit() is ordered behind the work already enqueued on torch's CURRENT
    stream of `device` at that moment (also when that is the default/null stream), so pixels produced by torch
    kernels need no host synchronisation; join() makes that stream wait for the outputs.  `stream="own"`: a
    private stream, the caller synchronises.  Anything else: a hipStream_t handle."""

    def __init__(self, device=0, stream="torch"):
        self.lib = _lib.load()
        self.device = device
        self._follow_torch = stream == "torch"
        h = C.c_void_p()
        if stream == "torch":
            with torch.cuda.device(device):
                sptr = torch.cuda.current_stream().cuda_stream
            check(self.lib.fpng_amd_encoder_create_on_stream(C.byref(h), device, C.c_void_p(sptr) if sptr else None))
        elif stream is None or stream == "own":
            check(self.lib.fpng_amd_encoder_create(C.byref(h), device, None))
        else:
            check(self.lib.fpng_amd_encoder_create_on_stream(C.byref(h), device, C.c_void_p(int(stream))))
        self.h = h
        self._keep = {}  # ticket -> buffers of that submission (at most 8 are in flight: the C side's slot ring)

    @property
    def lanes(self):
        """Lanes (stream + scratch set each) this encoder's submissions take turns over: fixed when it was created."""
        return int(self.lib.fpng_amd_encoder_lanes(self.h))

    def _sync_stream(self):
        if self._follow_torch:
            with torch.cuda.device(self.device):
                sptr = torch.cuda.current_stream().cuda_stream
            check(self.lib.fpng_amd_encoder_set_stream(self.h, C.c_void_p(sptr) if sptr else None))

    def close(self):
        if getattr(self, "h", None):
            self.lib.fpng_amd_encoder_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- device-resident batch: the hot path ----
    @staticmethod
    def make_batch(images, outs):
        """Descriptor array (fpng_amd_image[n]) for a list of image / output tensors.  Build it once when the
        same buffers are encoded repeatedly (a capture pipeline): submit() then costs one C call."""
        _need_cuda("make_batch", images, "images")
        return (images, outs, _source_records("make_batch", images, "image", outs)[0])

    def _submit(self, call, n, keep):
        """What every submit method ends in: call(ticket) is its one C call; `keep` -- the descriptor, and whatever else the GPU
        reads or writes -- stays alive while the submission can be in flight.  Returns n."""
        self._sync_stream()
        t = C.c_uint64(0)
        check(call(C.byref(t)))
        self.last_ticket = t.value
        # a submission 8 tickets back has finished (its slot was reused)
        self._keep[t.value] = keep
        for old in [k for k in self._keep if k + 8 <= t.value]:
            del self._keep[old]
        return n

    def submit(self, images, outs=None, flags=0):
        """images: list of uint8 CUDA tensors shaped (h, w, c), contiguous, and outs: list of uint8 CUDA
        tensors with >= max_encoded_size bytes -- or images = a make_batch() descriptor and outs = None.
        Asynchronous; call finish() for the sizes."""
        batch = _own_batch("submit", "make_batch", images, Image) if outs is None else self.make_batch(images, outs)
        n = len(batch[2])
        return self._submit(lambda t: self.lib.fpng_amd_encode_submit(self.h, batch[2], n, flags, t), n, batch)

    @staticmethod
    def make_batch_ex(images, outs, order="rgb", bottom_up=False):
        """Descriptor array (fpng_amd_image_ex[n]) for submit_ex(): uint8 CUDA tensor VIEWS (h, w, c) in place -- crops, BGR(A),
        [..., :3] of RGBA, bottom-up buffers -- described by source_layout(view, order, bottom_up) (order / bottom_up: one value, or
        one per image).  outs: uint8 CUDA tensors of >= max_encoded_size(w, h, c) bytes."""
        _need_cuda("make_batch_ex", images, "images")
        _need_cuda("make_batch_ex", outs, "outs")
        return (images, outs, _source_records("make_batch_ex", images, "ex", outs, order, bottom_up)[0])

    def submit_ex(self, images, outs=None, flags=0, order="rgb", bottom_up=False):
        """submit() for images in other layouts (fpng_amd_encode_submit_ex): images = tensor views as for make_batch_ex() with outs,
        or a make_batch_ex() descriptor and outs = None.  The files are the ones submit() writes for the same pixels repacked as
        R,G,B[,A].  Asynchronous; wait(last_ticket, n) / finish() for the sizes."""
        batch = _own_batch("submit_ex", "make_batch_ex", images, ImageEx) if outs is None else self.make_batch_ex(images, outs, order, bottom_up)
        n = len(batch[2])
        return self._submit(lambda t: self.lib.fpng_amd_encode_submit_ex(self.h, batch[2], n, flags, t), n, batch)

    @staticmethod
    def make_batch_planar(images, outs, order="rgb", bottom_up=False):
        """Descriptor array (fpng_amd_image_planar[n]) for submit_planar(): uint8 tensor VIEWS shaped (c, h, w) -- channels first, as
        torch holds images -- encoded where they lie, described by source_layout_planar(view, order, bottom_up) (order / bottom_up: one
        value, or one per image).  list(nchw_batch) is a valid `images`.  outs: uint8 tensors of >= max_encoded_size(w, h, c) bytes."""
        return (images, outs, _source_records("make_batch_planar", images, "planar", outs, order, bottom_up)[0])

    def submit_planar(self, images, outs=None, flags=0, order="rgb", bottom_up=False):
        """submit() for planar (c, h, w) images (fpng_amd_encode_submit_planar): images = CUDA tensor views as for make_batch_planar()
        with outs, or a make_batch_planar() descriptor and outs = None.  The files are the ones submit() writes for the same pixels
        interleaved as R,G,B[,A] -- without the permute(1, 2, 0).contiguous() copy.  Asynchronous; wait(last_ticket, n) / finish()
        for the sizes."""
        batch = _own_batch("submit_planar", "make_batch_planar", images, ImagePlanar) if outs is None else self.make_batch_planar(images, outs, order, bottom_up)
        _need_cuda("submit_planar", [*batch[0], *batch[1]], "images and outs")
        n = len(batch[2])
        return self._submit(lambda t: self.lib.fpng_amd_encode_submit_planar(self.h, batch[2], n, flags, t), n, batch)

    @staticmethod
    def make_batch_float(images, outs, order="rgb", bottom_up=False, mean=None, std=None, scale=None, bias=None):
        """Descriptor (images, outs, fpng_amd_image_planar[n], fpng_amd_float_format) for submit_float(): float32 / float16 /
        bfloat16 tensor VIEWS shaped (c, h, w) -- all of ONE dtype -- encoded where they lie, described by
        source_layout_float(view, order, bottom_up) (order / bottom_up: one value, or one per image).  A byte of the file's channel c
        (R, G, B, A, whatever the planes' order in memory) is rint(fmaf(x, scale[c], bias[c])) clamped to [0, 255], NaN giving 0: give
        mean and std (denormalize_constants(): (x * std + mean) * 255), or scale and bias (up to four values each, padded with 255
        and 0), or neither for plain [0, 1] values.  list(nchw_batch) is a valid `images`."""
        return (images, outs) + _source_records("make_batch_float", images, "float", outs, order, bottom_up, mean, std, scale, bias)

    def submit_float(self, images, outs=None, flags=0, order="rgb", bottom_up=False, mean=None, std=None, scale=None, bias=None):
        """submit_planar() for float (c, h, w) images (fpng_amd_encode_submit_planar_float): images = CUDA tensor views as for
        make_batch_float() with outs, or a make_batch_float() descriptor and outs = None.  The files are the ones submit_planar()
        writes for x.mul(scale).add(bias).round().clamp(0, 255).to(torch.uint8) -- without those passes and the uint8 image between
        them.  Asynchronous; wait(last_ticket, n) / finish() for the sizes."""
        if outs is None:
            batch = _own_batch("submit_float", "make_batch_float", images, ImagePlanar, size=4)
        else:
            batch = self.make_batch_float(images, outs, order, bottom_up, mean, std, scale, bias)
        _need_cuda("submit_float", [*batch[0], *batch[1]], "images and outs")
        n = len(batch[2])
        return self._submit(lambda t: self.lib.fpng_amd_encode_submit_planar_float(self.h, batch[2], n, C.byref(batch[3]), flags, t), n, batch)

    @staticmethod
    def make_batch_packed(images, kind="image", **layout):
        """Descriptor for submit_packed(): the make_batch*() descriptor of `kind` ("image" | "ex" | "planar" | "float", with that
        kind's layout arguments: order, bottom_up, and for "float" mean / std / scale / bias) without outputs."""
        if kind == "image" and layout:
            raise ValueError(f"make_batch_packed: kind 'image' takes no layout arguments, got {sorted(layout)}")
        if kind in ("ex", "planar") and set(layout) - {"order", "bottom_up"}:  # (what that kind's own maker has no argument for)
            raise TypeError(f"make_batch_packed: kind {kind!r} takes order and bottom_up, got {sorted(layout)}")
        if kind == "ex":
            _need_cuda("make_batch_packed", images, "images")  # (as make_batch_ex asks)
        arr, fmt = _source_records("make_batch_packed", images, kind, **layout)
        return ("packed", kind, images, [_NoOut] * len(images), arr) + ((fmt,) if kind == "float" else ())

    def submit_packed(self, images, arena, kind="image", align=16, lead=0, table=None, flags=0, **layout):
        """fpng_amd_encode_submit_packed: the files of ONE submission back to back in `arena` (a uint8 CUDA tensor whose address is a
        multiple of align), placed on the GPU from their actual sizes: every file at round_up(cursor, align) + lead, `lead` bytes
        in front of it left untouched; a file that finds no room gets status STATUS_ARENA_FULL and not a byte of it is written
        (pack_place() is the rule, pack_capacity() the size that refuses nothing).  images: tensors as for submit / submit_ex /
        submit_planar / submit_float (kind, **layout: that call's order / bottom_up / mean / std / scale / bias), or a
        make_batch_packed() descriptor.  table: optional int64 CUDA tensor of 2 * (n + 1) elements, filled with {offset, png_size} per
        file and {total, files placed}.  Asynchronous; wait_packed(last_ticket, n) for the records."""
        if isinstance(images, tuple) and images[:1] == ("packed",):
            batch = images
        elif isinstance(images, tuple) and any(isinstance(v, C.Array) for v in images):
            raise ValueError("submit_packed: a descriptor comes from make_batch_packed(), not from another call's maker")
        else:
            batch = self.make_batch_packed(images, kind, **layout)
        kind, arr = batch[1], batch[4]
        n = len(arr)
        pack = _pack_record("submit_packed", arena, align, lead, table, n)
        _need_cuda("submit_packed", batch[2], "images")
        fmt = C.byref(batch[5]) if kind == "float" else None
        # (the arena and the table stay alive with the sources)
        return self._submit(lambda t: self.lib.fpng_amd_encode_submit_packed(self.h, _DESC_KINDS[kind], C.cast(arr, C.c_void_p), n, fmt, flags, C.byref(pack), t),
                            n, (batch, arena, table))

    def wait_packed(self, ticket, n):
        """Waits for the packed submission `ticket`; returns ([(offset, png_size, mode, status)], total): file i is
        arena[offset:offset + png_size], total the end of the last file placed."""
        res = (_lib.PackedResult * n)()
        total = C.c_uint64(0)
        check(self.lib.fpng_amd_encode_wait_packed(self.h, ticket, res, n, C.byref(total)))
        self._keep.pop(ticket, None)
        return [(r.offset, r.png_size, r.mode, r.status) for r in res], total.value

    def encode_packed(self, images, kind="image", align=16, lead=0, flags=0, **layout):
        """Convenience: an arena of pack_capacity() bytes, one packed submission, the wait: returns (arena[:total], records) --
        records as wait_packed() gives them; one .cpu() of the first and one write() make a shard body."""
        batch = self.make_batch_packed(images, kind, **layout)
        arr = batch[4]
        dims = [(a.w, a.h, c) for a, c in zip(arr, _record_channels(kind, arr))]
        cap = pack_capacity(dims, align, lead)
        a = max(int(align), 16)
        raw = torch.empty(cap + a, dtype=torch.uint8, device=batch[2][0].device)
        skip = (-raw.data_ptr()) % a
        arena = raw[skip:skip + cap]
        n = self.submit_packed(batch, arena, align=align, lead=lead, flags=flags)
        records, total = self.wait_packed(self.last_ticket, n)
        return arena[:total], records

    def submit_renditions(self, images, renditions, kind="image", outs=None, arena=None, flags=0, align=16, lead=0, table=None, **layout):
        """fpng_amd_encode_submit_renditions: resized copies of device images, one file per fpng_amd.rendition() record, in ONE
        submission -- img.crop(box).resize(size, filter) as Pillow computes it, encoded as submit() encodes those pixels.  images:
        CUDA tensors as for submit / submit_ex / submit_planar / submit_float (kind "image" | "ex" | "planar" | "float", **layout:
        that call's order / bottom_up / mean / std / scale / bias), read where they lie.  Either outs -- one uint8 CUDA tensor of
        >= max_encoded_size(w, h, c) bytes per rendition -- or arena (with align, lead, table as for submit_packed): the files
        back to back in it, in rendition order.  Asynchronous; wait(last_ticket, n) for the (png_size, mode, status) records, with
        an arena wait_packed(last_ticket, n).  Returns the number of renditions."""
        if (outs is None) == (arena is None):
            raise ValueError("submit_renditions: outs (one per rendition) or arena, one of the two")
        images = list(images)
        _need_cuda("submit_renditions", images, "images")
        arr, fmt = _source_records("submit_renditions", images, kind, **layout)
        rarr = _rendition_records(renditions)
        n = len(rarr)
        pack = None
        if outs is not None:
            if len(outs) != n or not all(o.is_cuda and o.dtype == torch.uint8 and o.is_contiguous() for o in outs):
                raise ValueError("submit_renditions: outs are contiguous uint8 CUDA tensors, one per rendition")
            for r, o in zip(rarr, outs):
                r.d_out, r.out_cap = o.data_ptr(), o.numel()
        else:
            pack = C.byref(_pack_record("submit_renditions", arena, align, lead, table, n))
        fmt = C.byref(fmt) if fmt is not None else None
        # (sources and destinations stay alive while the submission runs)
        return self._submit(lambda t: self.lib.fpng_amd_encode_submit_renditions(self.h, _DESC_KINDS[kind], C.cast(arr, C.c_void_p), len(arr), fmt, rarr, n, flags, pack, t),
                            n, (images, outs, arena, table))

    def encode_renditions(self, images, renditions, kind="image", flags=0, **layout):
        """Convenience: outputs of max_encoded_size() each, one submit_renditions(), the wait: the files as a list of bytes, in
        rendition order."""
        images = list(images)
        chans = _record_channels(kind, _source_records("encode_renditions", images, kind, **layout)[0])
        for r in renditions:
            if r.image >= len(images):
                raise ValueError(f"encode_renditions: rendition of image {r.image} of {len(images)}")
        outs = [torch.empty(max_encoded_size(r.w, r.h, chans[r.image]) + 64, dtype=torch.uint8, device=images[r.image].device) for r in renditions]
        n = self.submit_renditions(images, renditions, kind=kind, outs=outs, flags=flags, **layout)
        return _files(outs, self.wait(self.last_ticket, n))

    @staticmethod
    def make_batch_yuv(frames, outs=None, surface="nv12", matrix=None, standard="bt709", full_range=False):
        """Descriptor ("yuv", frames, outs, fpng_amd_yuv_frame[n], fpng_amd_yuv_format) for submit_yuv(): build it once when the same
        surfaces are encoded repeatedly (a decoder's ring of frames); submit_yuv(descriptor) then costs one C call.  outs: one
        uint8 CUDA tensor of >= max_encoded_size(w, h, 3) bytes per frame, or None for a call with an arena or with renditions."""
        frames, arr = _yuv_records("make_batch_yuv", frames, surface, outs)
        return ("yuv", frames, outs, arr, _yuv_format("make_batch_yuv", surface, matrix, standard, full_range))

    def submit_yuv(self, frames, outs=None, arena=None, renditions=None, surface="nv12", matrix=None, standard="bt709", full_range=False, flags=0, align=16,
                   lead=0, table=None):
        """fpng_amd_encode_submit_yuv: video frames as the decoder left them -- "nv12", "p016" (P010 / P012 too), "yuv444",
        "yuv444_16" -- encoded as 3-channel files in ONE submission, the conversion inside the row walk: no RGB image exists in
        memory.  frames: a tuple of CUDA tensor views per frame, as yuv_frame_layout() takes them.  matrix: a (3, 4) array, or None
        for yuv_matrix(standard, full_range).  4:2:0 chroma is replicated, not interpolated.  Without renditions every frame is a
        file: outs -- one uint8 CUDA tensor of >= max_encoded_size(w, h, 3) bytes per frame -- or arena (with align, lead, table as
        for submit_packed).  With renditions (fpng_amd.rendition() records whose `image` indexes the frames) the files are the
        renditions', as submit_renditions() writes them for the converted frames: outs, one per rendition, or arena.
        frames may also be a make_batch_yuv() descriptor (its outs, surface and matrix then hold, and outs here stays None unless
        the files are renditions').  Asynchronous; wait(last_ticket, n) for the (png_size, mode, status) records, with an arena
        wait_packed(last_ticket, n).  Returns the number of files."""
        if isinstance(frames, tuple) and frames[:1] == ("yuv",):
            _, frames, own_outs, arr, fmt = frames
            if own_outs is not None:
                if outs is not None or arena is not None or renditions is not None:
                    raise ValueError("submit_yuv: a descriptor with outs is a whole call: no outs, arena or renditions beside it")
                outs = own_outs
        else:
            frames, arr = _yuv_records("submit_yuv", frames, surface, outs if renditions is None else None)
            fmt = _yuv_format("submit_yuv", surface, matrix, standard, full_range)
        if (outs is None) == (arena is None):
            raise ValueError("submit_yuv: outs (one per file) or arena, one of the two")
        _need_cuda("submit_yuv", [p for f in frames for p in f], "the frames' planes")
        rarr = _rendition_records(renditions) if renditions is not None else None
        n = len(arr) if rarr is None else len(rarr)
        pack = None
        if outs is not None:
            if len(outs) != n or not all(o.is_cuda and o.dtype == torch.uint8 and o.is_contiguous() for o in outs):
                raise ValueError("submit_yuv: outs are contiguous uint8 CUDA tensors, one per file")
            for r, o in zip(rarr if rarr is not None else (), outs):
                r.d_out, r.out_cap = o.data_ptr(), o.numel()
        else:
            pack = C.byref(_pack_record("submit_yuv", arena, align, lead, table, n))
        # (sources and destinations stay alive while the submission runs)
        return self._submit(lambda t: self.lib.fpng_amd_encode_submit_yuv(self.h, arr, len(arr), C.byref(fmt), rarr, 0 if rarr is None else len(rarr), flags, pack, t),
                            n, (frames, outs, arena, table))

    def encode_yuv(self, frames, renditions=None, surface="nv12", matrix=None, standard="bt709", full_range=False, flags=0):
        """Convenience: outputs of max_encoded_size() each, one submit_yuv(), the wait: the files as a list of bytes -- one per frame,
        or one per rendition, in their order."""
        frames = [tuple(f) for f in frames]
        if renditions is None:
            dims = [tuple(yuv_frame_layout(f, surface)[3:]) for f in frames]
        else:
            dims = [(r.w, r.h) for r in renditions]
        dev = frames[0][0].device
        outs = [torch.empty(max_encoded_size(w, h, 3) + 64, dtype=torch.uint8, device=dev) for w, h in dims]
        n = self.submit_yuv(frames, outs=outs, renditions=renditions, surface=surface, matrix=matrix, standard=standard, full_range=full_range, flags=flags)
        return _files(outs, self.wait(self.last_ticket, n))

    def wait(self, ticket, n):
        """Waits for the submission `ticket` (see last_ticket) only; returns its (png_size, mode, status) records."""
        res = (Result * n)()
        check(self.lib.fpng_amd_encode_wait(self.h, ticket, res, n))
        self._keep.pop(ticket, None)
        return [(r.png_size, r.mode, r.status) for r in res]

    def query(self, ticket):
        rc = self.lib.fpng_amd_encode_query(self.h, ticket)
        if rc < 0:
            check(rc)
        return bool(rc)

    def phase_names(self):
        """Names of the kernels/phases of the last submission's pipeline (see last_phase_ms)."""
        return self.lib.fpng_amd_encoder_phase_names(self.h).decode().split(",")

    def join(self):
        """Device-side join: the encoder's stream (torch's current one for stream="torch") waits for every
        submission made so far (no host wait)."""
        self._sync_stream()
        check(self.lib.fpng_amd_encoder_join(self.h))

    def finish(self, n):
        """Waits for ALL submissions in flight; returns (png_size, mode, status) of the last one's n images."""
        res = (Result * n)()
        check(self.lib.fpng_amd_encode_finish(self.h, res, n))
        self._keep = {}
        return [(r.png_size, r.mode, r.status) for r in res]

    def encode_tensors(self, images, flags=0, submissions=1):
        """Convenience: allocate outputs, encode, return list of PNG byte strings.  submissions: the batch goes to the GPU in that
        many submissions (at most one per image).  With frames in hand and nothing in flight, four submissions beat one -- their
        chains run on different lanes, one's assemble next to the next one's row walk: 8 x 8K 0.66 -> 0.56 ms, 64 x 1080p RGB
        0.34 -> 0.31 ms (tools/oneshot_split.py, profiles/r05_hw_queues.txt section 6); a caller that keeps submissions in flight
        anyway gains nothing from smaller ones."""
        outs = [torch.empty(max_encoded_size(im.shape[1], im.shape[0], im.shape[2]) + 64, dtype=torch.uint8,
                            device=im.device) for im in images]
        n = len(images)
        subs = min(max(1, submissions), 8)  # (the C side keeps the records of the last eight submissions)
        k = max(1, (n + subs - 1) // subs)
        parts = []
        for i in range(0, n, k):
            self.submit(images[i:i + k], outs[i:i + k], flags)
            parts.append((self.last_ticket, len(images[i:i + k])))
        res = []
        for ticket, m in parts:
            res += self.wait(ticket, m)
        return _files(outs, res), [m for _, m, _ in res]

    def decode_batch(self, pngs, desired_chans, dims=None):
        """fpng_amd_decode_batch: list of fpng-written files (bytes) -> list of (status, uint8 CUDA tensor (h, w, desired_chans)
        or None, channels_in_file).  Output buffers are sized from the files' headers (dims: optional list of (w, h) to skip that)."""
        import struct
        n = len(pngs)
        arr = (_lib.PngIn * n)()
        res = (_lib.DecodeResult * n)()
        device_data, keep = _file_records("decode_batch", pngs, arr)  # (keep: alive until the call has returned)
        if device_data:
            raise ValueError("decode_batch: the files are in device memory (decode_device)")
        outs = []
        for i, p in enumerate(pngs):
            w, h = dims[i] if dims else ((struct.unpack(">II", bytes(p[16:24]))) if len(p) >= 24 else (0, 0))
            cap = w * h * desired_chans if 0 < w <= (1 << 24) and 0 < h <= (1 << 24) and w * h <= (1 << 30) else 0
            t = torch.empty(max(cap, 16), dtype=torch.uint8, device=f"cuda:{self.device}")
            outs.append(t)
            arr[i].d_pixels = t.data_ptr()
            arr[i].pixels_cap = t.numel()
        self._sync_stream()
        check(self.lib.fpng_amd_decode_batch(self.h, arr, n, desired_chans, res))
        out = []
        for i in range(n):
            r = res[i]
            ok = r.status == 0
            out.append((r.status, outs[i][: r.w * r.h * desired_chans].view(r.h, r.w, desired_chans) if ok else None, r.channels_in_file))
        return out

    def make_decode_batch(self, pngs, desired_chans, dims, outs=None):
        """Descriptor (fpng_amd_png_in[n] + the result records) for decode_device().  Build it once when the same device buffers are
        decoded repeatedly: a call then costs one C call, as make_batch() does for submit() -- filling the array takes Python about
        3 us a file, as long as the GPU needs for a 512 x 512 one."""
        n = len(pngs)
        arr = (_lib.PngIn * n)()
        res = (_lib.DecodeResult * n)()
        made = []
        for i, p in enumerate(pngs):
            w, h = dims[i]
            t = outs[i] if outs is not None else torch.empty(max(w * h * desired_chans, 16), dtype=torch.uint8, device=f"cuda:{self.device}")
            made.append(t)
            arr[i].data = p.data_ptr() if p.numel() else None
            arr[i].size = p.numel()
            arr[i].d_pixels = t.data_ptr()
            arr[i].pixels_cap = t.numel()
        return DecodeBatch(list(pngs), made, arr, res, desired_chans)

    def decode_device(self, pngs, desired_chans=None, dims=None, outs=None, results=True):
        """fpng_amd_decode_batch_device: list of uint8 CUDA tensors holding whole fpng-written files (e.g. the encoder's outputs) ->
        list of (status, uint8 CUDA tensor (h, w, desired_chans) or None, channels_in_file).  dims: list of (w, h) (sizes the
        output tensors; the files' bytes stay on the device); outs: optional preallocated uint8 CUDA tensors to decode into.
        pngs may be a make_decode_batch() descriptor (the other arguments are then its own); results=False: the call returns the
        descriptor, whose statuses() / results() can be asked later."""
        batch = pngs if isinstance(pngs, DecodeBatch) else self.make_decode_batch(pngs, desired_chans, dims, outs)
        self._sync_stream()
        check(self.lib.fpng_amd_decode_batch_device(self.h, batch.arr, len(batch.arr), batch.desired_chans, batch.res))
        return batch.results() if results else batch

    def make_decode_batch_png(self, pngs, desired_chans=4, dims=None, outs=None, flags=0):
        """Descriptor (fpng_amd_png[n] + the result records) for decode_device_png() / decode_batch_png(): ordinary PNG files --
        uint8 CUDA tensors holding whole files, or bytes-like objects in host memory, one kind per batch.  dims: list of (w, h)
        that sizes the output tensors (default: read from the files' headers); outs: preallocated contiguous uint8 CUDA tensors
        of at least w * h * desired_chans elements to decode into instead."""
        import struct
        who = "make_decode_batch_png"
        n = len(pngs)
        if desired_chans not in (3, 4):
            raise ValueError(f"{who}: desired_chans is 3 or 4")
        if outs is not None and len(outs) != n:
            raise ValueError(f"{who}: {n} files, {len(outs)} destinations")
        arr = (_lib.PngIn * n)()
        res = (_lib.DecodeResult * n)()
        device_data, keep = _file_records(who, pngs, arr)
        if outs is None and dims is None:
            if device_data:  # (the headers' 24 bytes, one copy for the batch)
                heads = torch.stack([torch.nn.functional.pad(p[:24], (0, max(0, 24 - p.numel()))) for p in pngs]).cpu().numpy() if n else np.zeros((0, 24), np.uint8)
                dims = [struct.unpack(">II", heads[i, 16:24].tobytes()) for i in range(n)]
            else:
                dims = [struct.unpack(">II", bytes(p[16:24])) if len(p) >= 24 else (0, 0) for p in pngs]
        made = []
        for i in range(n):
            if outs is not None:
                t = outs[i]
                if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()):
                    raise ValueError(f"{who}: the destinations are contiguous uint8 CUDA tensors")
            else:
                w, h = dims[i]
                cap = w * h * desired_chans if 0 < w <= (1 << 24) and 0 < h <= (1 << 24) and w * h <= (1 << 30) else 0
                t = torch.empty(max(cap, 16), dtype=torch.uint8, device=f"cuda:{self.device}")
            made.append(t)
            arr[i].d_pixels, arr[i].pixels_cap = t.data_ptr(), t.numel()
        return DecodeBatchPng(list(pngs), made, arr, res, device_data, keep, desired_chans=desired_chans, flags=flags)

    def _decode_png(self, device_data, pngs, desired_chans, dims, outs, flags, results):
        return self._run_decode(DecodeBatchPng, device_data, pngs, lambda who: self.make_decode_batch_png(pngs, desired_chans, dims, outs, flags),
                                lambda b: ("fpng_amd_decode_batch_device_png" if device_data else "fpng_amd_decode_batch_png", [b.arr, len(b.arr), b.desired_chans, b.flags, b.res]),
                                results)

    def decode_device_png(self, pngs, desired_chans=4, dims=None, outs=None, flags=0, results=True):
        """fpng_amd_decode_batch_device_png: ordinary PNG files (8-bit grey, grey + alpha, RGB, palette, RGBA; any zlib stream, all
        five filters, any number of IDAT chunks) in uint8 CUDA tensors -> list of (status, uint8 CUDA tensor (h, w, desired_chans)
        or None, channels_in_file).  fpng-written files of the batch take the fpng path unless flags has FPNG_AMD_PNG_GENERAL_ONLY;
        FPNG_AMD_DECODE_UNSUPPORTED_PNG: a valid PNG outside this tier (other bit depths, interlace, unknown critical chunks).
        pngs may be a make_decode_batch_png() descriptor; results=False returns the descriptor."""
        return self._decode_png(True, pngs, desired_chans, dims, outs, flags, results)

    def decode_batch_png(self, pngs, desired_chans=4, dims=None, outs=None, flags=0, results=True):
        """fpng_amd_decode_batch_png: decode_device_png() for files in host memory (bytes-like objects), uploaded in groups."""
        return self._decode_png(False, pngs, desired_chans, dims, outs, flags, results)

    def last_decode_png_kernel_ms(self):
        """with profiling on: (inflate ms, un-filter ms) of the last decode_*_png call's first group of general-tier files"""
        ms = (C.c_float * 2)()
        check(self.lib.fpng_amd_decode_png_last_kernel_ms(self.h, ms))
        return float(ms[0]), float(ms[1])

    @staticmethod
    def make_decode_batch_ex(pngs, outs, order="rgb", bottom_up=False):
        """Descriptor (fpng_amd_png_ex[n] + the result records) for decode_device_ex() / decode_batch_ex(): the files -- uint8 CUDA
        tensors holding whole files, or bytes-like objects in host memory, one kind per batch -- and uint8 (h, w, c) tensor VIEWS on
        the device that the pixels are decoded into where they lie: crops, BGR(A), *X, bottom-up buffers, described by
        dest_layout(view, order, bottom_up) (order / bottom_up: one value, or one per file).  Size every view to its file: the
        call's room check (pixels_cap) is the span from the view's first byte to its last, so a file with more rows or more bytes
        than that is refused (FPNG_AMD_ERR_BUFFER_TOO_SMALL), but a shorter, wider one would write between the view's rows.
        Build it once when the same buffers are decoded repeatedly."""
        who = "make_decode_batch_ex"
        n = len(pngs)
        if len(outs) != n:
            raise ValueError(f"{who}: {n} files, {len(outs)} destinations")
        orders, ups = _per_file(who, n, order, "plane orders"), _per_file(who, n, bottom_up, "bottom_up flags")
        arr = (_lib.PngExIn * n)()
        res = (_lib.DecodeResult * n)()
        device_data, keep = _file_records(who, pngs, arr)
        for i, t in enumerate(outs):
            if not (isinstance(t, torch.Tensor) and t.is_cuda):
                raise ValueError(f"{who}: the destinations are CUDA tensors")
            ptr, rp, fmt = dest_layout(t, orders[i], ups[i])
            h, w, _ = t.shape
            arr[i].format, arr[i].d_pixels, arr[i].row_pitch = fmt, ptr, rp
            arr[i].pixels_cap = (h - 1) * abs(rp) + w * dest_bytes(fmt)  # (the view's own rows: nothing around them)
        return DecodeBatchEx(list(pngs), list(outs), arr, res, device_data, keep)

    def _run_decode(self, cls, device_data, pngs, make, entry, results):
        """What every decode call into views does.  cls: the call's descriptor class; pngs: such a descriptor, or the files, of which
        make(who) then builds one; entry(batch): the C entry point's name and its arguments behind the encoder."""
        who = cls.call(device_data)
        if isinstance(pngs, (DecodeBatch, _DecodeBatchViews)) and not isinstance(pngs, cls):
            raise ValueError(f"{who}: a {type(pngs).maker}() descriptor is another call's ({cls.maker}() makes this one's)")
        batch = pngs if isinstance(pngs, cls) else make(who)
        if batch.device_data != device_data:
            raise ValueError(f"{who}: the files are in " + (f"host memory ({cls.call(False)})" if device_data else f"device memory ({cls.call(True)})"))
        if not all(t.is_cuda for t in batch.tensors()):
            raise ValueError(f"{who}: the destinations are CUDA tensors")
        self._sync_stream()
        symbol, args = entry(batch)
        check(getattr(self.lib, symbol)(self.h, *args))
        return batch.results() if results else batch

    def _decode_ex(self, device_data, pngs, outs, order, bottom_up, results):
        return self._run_decode(DecodeBatchEx, device_data, pngs, lambda who: self.make_decode_batch_ex(pngs, outs, order, bottom_up),
                                lambda b: (_file_symbol("ex", device_data), [b.arr, len(b.arr), b.res]), results)

    def decode_device_ex(self, pngs, outs=None, order="rgb", bottom_up=False, results=True):
        """fpng_amd_decode_batch_device_ex: uint8 CUDA tensors holding whole files, decoded into the caller's device tensor views
        `outs` in place (make_decode_batch_ex() has the rules) -> list of (status, the caller's view or None, channels_in_file).
        pngs may be a make_decode_batch_ex() descriptor of device files (outs = None); results=False returns the descriptor."""
        return self._decode_ex(True, pngs, outs, order, bottom_up, results)

    def decode_batch_ex(self, pngs, outs=None, order="rgb", bottom_up=False, results=True):
        """fpng_amd_decode_batch_ex: files in host memory (bytes) decoded into the caller's device tensor views -- decode_device_ex()
        for host-resident files.  pngs may be a make_decode_batch_ex() descriptor of host files (outs = None)."""
        return self._decode_ex(False, pngs, outs, order, bottom_up, results)

    @staticmethod
    def make_decode_batch_planar(pngs, outs, order="rgb", bottom_up=False):
        """Descriptor (fpng_amd_png_planar[n] + the result records) for decode_device_planar() / decode_batch_planar(): the files --
        uint8 CUDA tensors holding whole files, or bytes-like objects in host memory, one kind per batch -- and uint8 (c, h, w)
        tensor VIEWS that the pixels are decoded into where they lie, a plane per channel, described by
        dest_layout_planar(view, order, bottom_up) (order / bottom_up: one value, or one per file).  c = the planes written, 3 or 4.
        Size every view to its file, as for make_decode_batch_ex(): pixels_cap is the view's own span.  Build it once when the same
        buffers are decoded repeatedly."""
        who = "make_decode_batch_planar"
        n = len(pngs)
        if len(outs) != n:
            raise ValueError(f"{who}: {n} files, {len(outs)} destinations")
        orders, ups = _per_file(who, n, order, "plane orders"), _per_file(who, n, bottom_up, "bottom_up flags")
        arr = (_lib.PngPlanarIn * n)()
        res = (_lib.DecodeResult * n)()
        device_data, keep = _file_records(who, pngs, arr)
        _planar_dests(arr, outs, orders, ups, True, None)
        return DecodeBatchPlanar(list(pngs), list(outs), arr, res, device_data, keep)

    def _decode_planar(self, device_data, pngs, outs, order, bottom_up, results):
        return self._run_decode(DecodeBatchPlanar, device_data, pngs, lambda who: self.make_decode_batch_planar(pngs, outs, order, bottom_up),
                                lambda b: (_file_symbol("planar", device_data), [b.arr, len(b.arr), b.res]), results)

    def decode_device_planar(self, pngs, outs=None, order="rgb", bottom_up=False, results=True):
        """fpng_amd_decode_batch_device_planar: uint8 CUDA tensors holding whole files, decoded into the caller's (c, h, w) device
        tensor views `outs` in place (make_decode_batch_planar() has the rules) -> list of (status, the caller's view or None,
        channels_in_file) -- without the permute(2, 0, 1).contiguous() copy behind a packed decode.  pngs may be a
        make_decode_batch_planar() descriptor of device files (outs = None); results=False returns the descriptor."""
        return self._decode_planar(True, pngs, outs, order, bottom_up, results)

    def decode_batch_planar(self, pngs, outs=None, order="rgb", bottom_up=False, results=True):
        """fpng_amd_decode_batch_planar: decode_device_planar() for files in host memory (bytes)."""
        return self._decode_planar(False, pngs, outs, order, bottom_up, results)

    @staticmethod
    def make_decode_batch_float(pngs, outs, order="rgb", bottom_up=False, mean=None, std=None, scale=None, bias=None):
        """Descriptor (fpng_amd_png_planar[n], the fpng_amd_float_format and the result records) for decode_device_float() /
        decode_batch_float(): the files as for make_decode_batch_planar(), and float32 / float16 / bfloat16 (c, h, w) tensor VIEWS --
        all of ONE dtype -- described by dest_layout_float(view, order, bottom_up).  An element of plane c is
        fmaf(byte, scale[c], bias[c]) of the FILE's channel c (R, G, B, A, whatever the planes' order in memory), rounded to the
        dtype: give mean and std (normalize_constants(): (byte / 255 - mean) / std), or scale and bias (up to four values each,
        padded with 1 / 255 and 0), or neither for plain [0, 1] values.  pixels_cap is the view's own span in bytes."""
        who = "make_decode_batch_float"
        n = len(pngs)
        if len(outs) != n:
            raise ValueError(f"{who}: {n} files, {len(outs)} destinations")
        _, fmt = _dest_format(who, outs, mean, std, scale, bias, always=True)
        orders, ups = _per_file(who, n, order, "plane orders"), _per_file(who, n, bottom_up, "bottom_up flags")
        arr = (_lib.PngPlanarIn * n)()
        res = (_lib.DecodeResult * n)()
        device_data, keep = _file_records(who, pngs, arr)
        _planar_dests(arr, outs, orders, ups, False, fmt)
        return DecodeBatchFloat(list(pngs), list(outs), arr, res, device_data, keep, fmt=fmt)

    def _decode_float(self, device_data, pngs, outs, order, bottom_up, mean, std, scale, bias, results):
        return self._run_decode(DecodeBatchFloat, device_data, pngs, lambda who: self.make_decode_batch_float(pngs, outs, order, bottom_up, mean, std, scale, bias),
                                lambda b: (_file_symbol("planar_float", device_data), [b.arr, len(b.arr), _fmt_ref(b), b.res]), results)

    def decode_device_float(self, pngs, outs=None, order="rgb", bottom_up=False, mean=None, std=None, scale=None, bias=None, results=True):
        """fpng_amd_decode_batch_device_planar_float: uint8 CUDA tensors holding whole files, decoded into the caller's float (c, h, w)
        device tensor views `outs` in place as normalised values (make_decode_batch_float() has the rules) -> list of (status, the
        caller's view or None, channels_in_file) -- without the x.to(dtype).sub(mean).div(std) pass behind decode_device_planar().
        pngs may be a make_decode_batch_float() descriptor of device files (outs = None); results=False returns the descriptor."""
        return self._decode_float(True, pngs, outs, order, bottom_up, mean, std, scale, bias, results)

    def decode_batch_float(self, pngs, outs=None, order="rgb", bottom_up=False, mean=None, std=None, scale=None, bias=None, results=True):
        """fpng_amd_decode_batch_planar_float: decode_device_float() for files in host memory (bytes)."""
        return self._decode_float(False, pngs, outs, order, bottom_up, mean, std, scale, bias, results)

    @staticmethod
    def make_decode_batch_crop(pngs, crops, outs, order="rgb", bottom_up=False, mean=None, std=None, scale=None, bias=None):
        """Descriptor (fpng_amd_png_planar[n], fpng_amd_crop[n], the fpng_amd_float_format if any and the result records) for
        decode_device_crop() / decode_batch_crop(): the files as for make_decode_batch_planar(); crops: a sequence of (x, y, w, h)
        in pixels of each file, top-down; outs: (c, h, w) tensor VIEWS whose (h, w) is the crop's (ValueError otherwise) -- uint8
        views, described by dest_layout_planar() (mean / std / scale / bias must then be absent), or float32 / float16 / bfloat16
        views of ONE dtype, described by dest_layout_float() with the constants of make_decode_batch_float().  Element (c, j, i) is
        what the full call writes at (c, y + j, x + i).  A crop that leaves its file's image is that file's status
        (DECODE_CROP_OUTSIDE), found by the call; pixels_cap is the view's own span in bytes."""
        who = "make_decode_batch_crop"
        n = len(pngs)
        if len(crops) != n or len(outs) != n:
            raise ValueError(f"{who}: {n} files, {len(crops)} crops, {len(outs)} destinations")
        is_u8, fmt = _dest_format(who, outs, mean, std, scale, bias)
        orders, ups = _per_file(who, n, order, "plane orders"), _per_file(who, n, bottom_up, "bottom_up flags")
        arr = (_lib.PngPlanarIn * n)()
        carr = (_lib.Crop * n)()
        res = (_lib.DecodeResult * n)()
        device_data, keep = _file_records(who, pngs, arr)
        _planar_dests(arr, outs, orders, ups, is_u8, fmt)
        for i, t in enumerate(outs):
            c = _crop_record(f"{who}: file {i}", crops[i], carr[i])
            if (t.shape[1], t.shape[2]) != (c.h, c.w):
                raise ValueError(f"{who}: destination {i} is {t.shape[2]} x {t.shape[1]}, its crop {c.w} x {c.h}")
        return DecodeBatchCrop(list(pngs), list(outs), arr, res, device_data, keep, crops=carr, fmt=fmt)

    def _decode_crop(self, device_data, pngs, crops, outs, dtype, order, bottom_up, mean, std, scale, bias, results):
        def make(who):
            dests = outs
            if dests is None:  # (c = 3 planes of the crop's size each; files with alpha lose it)
                dests = [torch.empty((3, int(c[3]), int(c[2])), dtype=_alloc_dtype(who, dtype), device=f"cuda:{self.device}") for c in crops]
            return self.make_decode_batch_crop(pngs, crops, dests, order, bottom_up, mean, std, scale, bias)

        return self._run_decode(DecodeBatchCrop, device_data, pngs, make,
                                lambda b: (_file_symbol("planar_crop", device_data), [b.arr, b.crops, len(b.arr), _fmt_ref(b), b.res]), results)

    def decode_device_crop(self, pngs, crops=None, outs=None, dtype=torch.uint8, order="rgb", bottom_up=False, mean=None, std=None, scale=None, bias=None,
                           results=True):
        """fpng_amd_decode_batch_device_planar_crop: uint8 CUDA tensors holding whole files, of each of which the crop (x, y, w, h)
        is decoded into the caller's (c, h, w) device tensor view in place (make_decode_batch_crop() has the rules) -> list of
        (status, the caller's view or None, channels_in_file) -- without the full decode and the t[:, y:y+h, x:x+w].contiguous()
        copy behind it.  outs=None allocates (3, h, w) tensors of `dtype` (default torch.uint8).  pngs may be a
        make_decode_batch_crop() descriptor of device files (crops = outs = None); results=False returns the descriptor."""
        return self._decode_crop(True, pngs, crops, outs, dtype, order, bottom_up, mean, std, scale, bias, results)

    def decode_batch_crop(self, pngs, crops=None, outs=None, dtype=torch.uint8, order="rgb", bottom_up=False, mean=None, std=None, scale=None, bias=None,
                          results=True):
        """fpng_amd_decode_batch_planar_crop: decode_device_crop() for files in host memory (bytes)."""
        return self._decode_crop(False, pngs, crops, outs, dtype, order, bottom_up, mean, std, scale, bias, results)

    @staticmethod
    def make_decode_batch_resize(pngs, crops, outs, mirror=False, order="rgb", bottom_up=False, mean=None, std=None, scale=None, bias=None):
        """Descriptor (fpng_amd_png_planar[n], fpng_amd_crop[n], fpng_amd_resize[n], the fpng_amd_float_format if any and the result
        records) for decode_device_resize() / decode_batch_resize(): the files and crops as for make_decode_batch_crop(); outs:
        (c, out_h, out_w) tensor VIEWS of any size from 1 x 1 up -- list(batch) of an (n, 3, 224, 224) tensor -- uint8, or float32 /
        float16 / bfloat16 of ONE dtype with the constants of make_decode_batch_float(); mirror: one bool, or one per file.  Each
        crop is resized to its view's size by Pillow's 8-bit antialiased bilinear rule, mirrored where
        asked, and written once.  The call refuses (FpngAmdError) an empty crop and one of more than 32 x its output size in w or h."""
        who = "make_decode_batch_resize"
        n = len(pngs)
        if len(crops) != n or len(outs) != n:
            raise ValueError(f"{who}: {n} files, {len(crops)} crops, {len(outs)} destinations")
        mirrors = _per_file(who, n, mirror, "mirror flags")
        is_u8, fmt = _dest_format(who, outs, mean, std, scale, bias)
        orders, ups = _per_file(who, n, order, "plane orders"), _per_file(who, n, bottom_up, "bottom_up flags")
        arr = (_lib.PngPlanarIn * n)()
        carr = (_lib.Crop * n)()
        sarr = (_lib.Resize * n)()
        res = (_lib.DecodeResult * n)()
        device_data, keep = _file_records(who, pngs, arr)
        _planar_dests(arr, outs, orders, ups, is_u8, fmt)
        for i, t in enumerate(outs):
            _crop_record(f"{who}: file {i}", crops[i], carr[i])
            _, oh, ow = t.shape
            sarr[i].out_w, sarr[i].out_h, sarr[i].flags, sarr[i].reserved = ow, oh, (RESIZE_MIRROR if mirrors[i] else 0), 0
        return DecodeBatchResize(list(pngs), list(outs), arr, res, device_data, keep, crops=carr, sizes=sarr, fmt=fmt)

    def _decode_resize(self, device_data, pngs, crops, outs, size, mirror, dtype, order, bottom_up, mean, std, scale, bias, results):
        def make(who):
            dests = outs
            if crops is None:
                raise ValueError(f"{who}: crops, an (x, y, w, h) per file")
            if dests is None:  # (c = 3 planes of the output size each; files with alpha lose it)
                if size is None:
                    raise ValueError(f"{who}: outs, or size=(out_h, out_w) to allocate them")
                oh, ow = (int(v) for v in size)
                dests = list(torch.empty((len(pngs), 3, oh, ow), dtype=_alloc_dtype(who, dtype), device=f"cuda:{self.device}"))
            return self.make_decode_batch_resize(pngs, crops, dests, mirror, order, bottom_up, mean, std, scale, bias)

        return self._run_decode(DecodeBatchResize, device_data, pngs, make,
                                lambda b: (_file_symbol("planar_resize", device_data), [b.arr, b.crops, b.sizes, len(b.arr), _fmt_ref(b), b.res]), results)

    def decode_device_resize(self, pngs, crops=None, outs=None, size=None, mirror=False, dtype=torch.uint8, order="rgb", bottom_up=False, mean=None, std=None,
                             scale=None, bias=None, results=True):
        """fpng_amd_decode_batch_device_planar_resize: uint8 CUDA tensors holding whole files, of each of which the crop (x, y, w, h)
        is decoded, resized to its (c, out_h, out_w) device tensor view's size, mirrored where asked and written in place, as bytes
        or as normalised floats (make_decode_batch_resize() has the rules) -> list of (status, the caller's view or None,
        channels_in_file) -- RandomResizedCrop + RandomHorizontalFlip + Normalize without the F.interpolate, flip and normalise
        passes behind decode_device_crop().  outs=None with size=(out_h, out_w) allocates one (n, 3, out_h, out_w) tensor of `dtype`
        and returns its slices.  pngs may be a make_decode_batch_resize() descriptor of device files; results=False returns it."""
        return self._decode_resize(True, pngs, crops, outs, size, mirror, dtype, order, bottom_up, mean, std, scale, bias, results)

    def decode_batch_resize(self, pngs, crops=None, outs=None, size=None, mirror=False, dtype=torch.uint8, order="rgb", bottom_up=False, mean=None, std=None,
                            scale=None, bias=None, results=True):
        """fpng_amd_decode_batch_planar_resize: decode_device_resize() for files in host memory (bytes)."""
        return self._decode_resize(False, pngs, crops, outs, size, mirror, dtype, order, bottom_up, mean, std, scale, bias, results)

    @staticmethod
    def make_decode_batch_resize_view(pngs, crops, outs, full, window=None, filter="bilinear", mirror=False, order="rgb", bottom_up=False, mean=None, std=None,
                                      scale=None, bias=None):
        """Descriptor (fpng_amd_png_planar[n], fpng_amd_crop[n], fpng_amd_resize_view[n], the fpng_amd_float_format if any and the
        result records) for decode_device_resize_view() / decode_batch_resize_view(): files, crops, destinations and constants as
        for make_decode_batch_resize().  full: (full_w, full_h), the size each crop is resized to, or one per file; window: the
        (x, y, w, h) of that resized image that is written, or one per file -- None: the whole of it; filter: "bilinear" or
        "bicubic" (FILTER_*), or one per file; mirror: one bool, or one per file.  A destination's (h, w) is its window's, else
        ValueError.  Resize(256) + CenterCrop(224): crop, full, window = center_crop_view(file_w, file_h, 256, 224).  The call
        refuses (FpngAmdError) an empty crop or window, a window that leaves the full size and a crop of more than 32 x (bicubic:
        16 x) the full size in w or h."""
        who = "make_decode_batch_resize_view"
        n = len(pngs)
        if len(crops) != n or len(outs) != n:
            raise ValueError(f"{who}: {n} files, {len(crops)} crops, {len(outs)} destinations")
        fulls, windows = _per_file(who, n, full, "full sizes"), _per_file(who, n, window, "windows")
        filters, mirrors = _per_file(who, n, filter, "filters"), _per_file(who, n, mirror, "mirror flags")
        is_u8, fmt = _dest_format(who, outs, mean, std, scale, bias)
        orders, ups = _per_file(who, n, order, "plane orders"), _per_file(who, n, bottom_up, "bottom_up flags")
        arr = (_lib.PngPlanarIn * n)()
        carr = (_lib.Crop * n)()
        varr = (_lib.ResizeView * n)()
        res = (_lib.DecodeResult * n)()
        device_data, keep = _file_records(who, pngs, arr)
        _planar_dests(arr, outs, orders, ups, is_u8, fmt)
        for i, t in enumerate(outs):
            _crop_record(f"{who}: file {i}", crops[i], carr[i])
            v = _view_record(who, fulls[i], windows[i], filters[i], bool(mirrors[i]), varr[i])
            _, oh, ow = t.shape
            if (oh, ow) != (v.h, v.w):
                raise ValueError(f"{who}: destination {i} is {ow} x {oh}, its window {v.w} x {v.h}")
        return DecodeBatchResizeView(list(pngs), list(outs), arr, res, device_data, keep, crops=carr, views=varr, fmt=fmt)

    def _decode_resize_view(self, device_data, pngs, crops, outs, full, window, filter, mirror, dtype, order, bottom_up, mean, std, scale, bias, results):
        def make(who):
            dests = outs
            if crops is None or full is None:
                raise ValueError(f"{who}: crops, an (x, y, w, h) per file, and full, the (full_w, full_h) they are resized to")
            if dests is None:  # (c = 3 planes of the window's size each; files with alpha lose it)
                n, where = len(pngs), dict(dtype=_alloc_dtype(who, dtype), device=f"cuda:{self.device}")
                if _VIEW_ARG["full sizes"](full) and _VIEW_ARG["windows"](window):  # one size: one (n, 3, h, w) tensor and its slices
                    dests = list(torch.empty((n, 3, *_window_hw(full, window)), **where))
                else:
                    dests = [torch.empty((3, *_window_hw(f_, w_)), **where) for f_, w_ in zip(_per_file(who, n, full, "full sizes"), _per_file(who, n, window, "windows"))]
            return self.make_decode_batch_resize_view(pngs, crops, dests, full, window, filter, mirror, order, bottom_up, mean, std, scale, bias)

        return self._run_decode(DecodeBatchResizeView, device_data, pngs, make,
                                lambda b: (_file_symbol("planar_resize_view", device_data), [b.arr, b.crops, b.views, len(b.arr), _fmt_ref(b), b.res]), results)

    def decode_device_resize_view(self, pngs, crops=None, outs=None, full=None, window=None, filter="bilinear", mirror=False, dtype=torch.uint8, order="rgb",
                                  bottom_up=False, mean=None, std=None, scale=None, bias=None, results=True):
        """fpng_amd_decode_batch_device_planar_resize_view: uint8 CUDA tensors holding whole files; of each the crop (x, y, w, h) is
        resized to full = (full_w, full_h) by `filter` ("bilinear" or "bicubic": Pillow's 8-bit rules) --
        never materialised -- and the window (x, y, w, h) of that image is written to its (c, h, w) device tensor view, mirrored
        where asked, as bytes or normalised floats (make_decode_batch_resize_view() has the rules) -> list of (status, the caller's
        view or None, channels_in_file).  Resize(256) + CenterCrop(224) + Normalize in one call: crops, full and window from
        center_crop_view().  Only the source pixels the window's taps reach are decoded (resize_view_source()).  outs=None
        allocates (3, h, w) tensors of `dtype`, one (n, 3, h, w) tensor's slices where all files share one size.  pngs may be a
        make_decode_batch_resize_view() descriptor of device files; results=False returns it."""
        return self._decode_resize_view(True, pngs, crops, outs, full, window, filter, mirror, dtype, order, bottom_up, mean, std, scale, bias, results)

    def decode_batch_resize_view(self, pngs, crops=None, outs=None, full=None, window=None, filter="bilinear", mirror=False, dtype=torch.uint8, order="rgb",
                                 bottom_up=False, mean=None, std=None, scale=None, bias=None, results=True):
        """fpng_amd_decode_batch_planar_resize_view: decode_device_resize_view() for files in host memory (bytes)."""
        return self._decode_resize_view(False, pngs, crops, outs, full, window, filter, mirror, dtype, order, bottom_up, mean, std, scale, bias, results)

    @staticmethod
    def make_decode_batch_views(pngs, crops, outs, full, window=None, filter="bilinear", mirror=False, order="rgb", bottom_up=False, mean=None, std=None,
                                scale=None, bias=None, color=None, post=None, warp=None, tone=None, enhance=None, alpha=None, resample=None):
        """Descriptor (fpng_amd_png_planar[n], the uint32[n] view counts, an fpng_amd_crop, fpng_amd_resize_view and fpng_amd_view_dest
        per view, the fpng_amd_float_format if any and the result records, one per file) for decode_device_views() /
        decode_batch_views(): make_decode_batch_resize_view() with one more level of nesting.  crops[i]: the list of file i's crops,
        one (x, y, w, h) per view, at least one; outs[i]: the list of its destinations, a (c, window h, window w) view each, all of
        one c per file and one dtype per call.  full, window, filter, mirror, order and bottom_up: one value for all views, or a list
        with an entry per file, each entry one value for the file's views or a list with a value per view.  Constants as for
        make_decode_batch_resize().  color: None, or the views' colour matrices (color_matrix() makes them) -- one (3, 4)
        array-like for all views, or a list per file of one per view; the descriptor then goes through
        fpng_amd_decode_batch(_device)_planar_views_color.  post: None, or the views' post-processing records (view_post() makes
        them) -- one for all views, a list with one per file, or a list per file of one per view; the descriptor then goes through
        fpng_amd_decode_batch(_device)_planar_views_post, with color's matrices or without.  warp: None, or the views' affine warp
        records (view_warp() makes them), nested as post's; the descriptor then goes through
        fpng_amd_decode_batch(_device)_planar_views_warp, with color's matrices and post's records or without.  tone: None, or the
        views' tone records (view_tone() makes them), nested as post's; the descriptor then goes through
        fpng_amd_decode_batch(_device)_planar_views_tone, with the others' records or without.  enhance: None, or the views' enhance
        records (view_enhance() makes them), nested as post's; the descriptor then goes through
        fpng_amd_decode_batch(_device)_planar_views_enhance, with the others' records or without.  alpha: None, or the views' alpha
        records (view_alpha() makes them), nested as post's; the descriptor then goes through
        fpng_amd_decode_batch(_device)_planar_views_alpha, with the others' records or without.  resample: None, or the views'
        RESAMPLE filters -- "nearest", "box", "hamming", "lanczos", None (the view's own filter=) or what view_resample() returns --
        nested as post's; the descriptor then goes through fpng_amd_decode_batch(_device)_planar_views_resample."""
        return _make_views_batch(_PLANAR_VIEWS, pngs, crops, outs, full, window, filter, mirror, order, bottom_up, mean, std, scale, bias,
                                 dict(color=color, post=post, warp=warp, tone=tone, enhance=enhance, alpha=alpha, resample=resample))

    def _decode_views(self, layout, device_data, pngs, crops, outs, full, window, filter, mirror, dtype, order, bottom_up, mean, std, scale, bias, results, stages):
        """a views call of either layout (_ViewsLayout), for files in device or host memory; stages: as _make_views_batch's"""
        if isinstance(pngs, layout.batch_cls) and any(v is not None for v in stages.values()):
            raise ValueError(f"{layout.batch_cls.call(device_data)}: a descriptor carries its own records of the stages {', '.join(k for k, _, _, _ in _VIEW_STAGES)} "
                             f"({layout.maker}(..., {', '.join(k + '=' for k, _, _, _ in _VIEW_STAGES)}))")

        def make(who):
            dests = outs
            if crops is None or full is None:
                raise ValueError(f"{who}: crops, a list of (x, y, w, h) per file, and full, the (full_w, full_h) they are resized to")
            if outs is None or any(o is None for o in outs):  # (each window's size with c = 3; files with alpha lose it)
                where = dict(dtype=_alloc_dtype(who, dtype), device=f"cuda:{self.device}")
                counts = [len(c) for c in crops]
                fulls, windows = _per_view(who, counts, full, "full sizes"), _per_view(who, counts, window, "windows")
                dests = [[torch.empty(layout.empty_shape(*_window_hw(f_, w_)), **where) for f_, w_ in zip(fulls[i], windows[i])] if outs is None or outs[i] is None else outs[i]
                         for i in range(len(crops))]
            return _make_views_batch(layout, pngs, crops, dests, full, window, filter, mirror, order, bottom_up, mean, std, scale, bias, stages)

        return self._run_decode(layout.batch_cls, device_data, pngs, make, lambda b: views_entry(layout.name, device_data, b), results)

    def decode_device_views(self, pngs, crops=None, outs=None, full=None, window=None, filter="bilinear", mirror=False, dtype=torch.uint8, order="rgb",
                            bottom_up=False, mean=None, std=None, scale=None, bias=None, results=True, color=None, post=None, warp=None, tone=None, enhance=None, alpha=None, resample=None):
        """fpng_amd_decode_batch_device_planar_views: SEVERAL views of each file -- uint8 CUDA tensors holding whole files -- from one
        decode of it: two 224 x 224 RandomResizedCrop views for contrastive training, two global and six 96 x 96 local ones for
        multi-crop.  crops[i] lists file i's crops; each is resized to its full size by its filter and its window written to its
        (c, h, w) device tensor view, mirrored where asked, as bytes or normalised floats: exactly what decode_device_resize_view()
        writes for that view alone (make_decode_batch_views() has the nesting rules) -> list, per file, of (status, the list of
        the caller's views or None, channels_in_file).  A file is decoded ONCE, the bounding rectangle of its views' source boxes
        (views_source()); two small views far apart decode everything between them, and listing the file twice in
        decode_device_resize_view() may then be cheaper.  outs=None (or None for a file) allocates (3, h, w) tensors of `dtype`.
        pngs may be a make_decode_batch_views() descriptor of device files; results=False returns it.
        color: None, or a colour matrix per view (one (3, 4) array-like for all, or a list per file of one per view; color_matrix()
        makes them from ColorJitter-style factors), applied between the resize's bytes and the normalisation --
        fpng_amd_decode_batch_device_planar_views_color: u_c = clamp(m[c] . (r, g, b, 1), 0, 255) in fp32 fused multiply-adds, then
        rint for uint8 or the fmaf of scale / bias; a fourth plane skips the matrix.  The identity gives exactly the call without.
        post: None, or a post-processing record per view (view_post() makes them: Gaussian blur, solarize, posterize; one for all
        views, one per file, or a list per file of one per view), applied to the colour step's bytes before the normalisation --
        fpng_amd_decode_batch_device_planar_views_post; a record without flags leaves its view exactly the call's without.
        warp: None, or an affine warp record per view (view_warp() makes them from Pillow's six AFFINE coefficients, affine_matrix()
        those from torchvision's angle / translate / scale / shear; nested as post's), applied to the mirrored window's bytes
        between the colour step and the blur -- fpng_amd_decode_batch_device_planar_views_warp: RandomRotation, RandomAffine and
        RandAugment's geometric operations as Image.transform(size, AFFINE, ...) does them, nearest or bilinear, with a fill colour;
        a record without flags leaves its view exactly the call's without.
        tone: None, or a tone record per view (view_tone() makes them: autocontrast, equalize or contrast about the view's own mean,
        as Pillow's ImageOps / ImageEnhance do them; nested as post's), applied to the bytes behind the colour step and the warp and
        in front of the blur -- fpng_amd_decode_batch_device_planar_views_tone; a record without an op leaves its view exactly the
        call's without.
        enhance: None, or an enhance record per view (view_enhance() makes them: brightness, color or sharpness as Pillow's
        ImageEnhance does them; nested as post's), applied to the bytes behind the tone operation and in front of the blur --
        fpng_amd_decode_batch_device_planar_views_enhance; a record without an op leaves its view exactly the call's without.
        alpha: None, or an alpha record per view (view_alpha() makes them; nested as post's): what the view does with the fourth
        plane of a 4-channel file, inside the resize and in front of every other stage -- "composite" over an opaque background
        colour as Image.alpha_composite does and then resize, or resize "premultiplied" as Image.resize of an RGBA image does --
        fpng_amd_decode_batch_device_planar_views_alpha; a record without an op, and any record on a 3-channel file, leaves its
        view exactly the call's without.
        resample: None, or a RESAMPLE filter per view -- "nearest", "box", "hamming" or "lanczos" (Pillow's Image.NEAREST, BOX,
        HAMMING, LANCZOS), None for the view's own filter=, or what view_resample() returns; one for all views, one per file, or a
        list per file of one per view -- which overrides the view's filter= in the resize:
        fpng_amd_decode_batch_device_planar_views_resample.  "nearest" is what a label map is resized with: give the mask the
        image's crops, windows, mirror flags and warp records.  A None leaves its view exactly the call's without."""
        return self._decode_views(_PLANAR_VIEWS, True, pngs, crops, outs, full, window, filter, mirror, dtype, order, bottom_up, mean, std, scale, bias, results,
                                  dict(color=color, post=post, warp=warp, tone=tone, enhance=enhance, alpha=alpha, resample=resample))

    def decode_batch_views(self, pngs, crops=None, outs=None, full=None, window=None, filter="bilinear", mirror=False, dtype=torch.uint8, order="rgb",
                           bottom_up=False, mean=None, std=None, scale=None, bias=None, results=True, color=None, post=None, warp=None, tone=None, enhance=None, alpha=None, resample=None):
        """fpng_amd_decode_batch_planar_views: decode_device_views() for files in host memory (bytes)."""
        return self._decode_views(_PLANAR_VIEWS, False, pngs, crops, outs, full, window, filter, mirror, dtype, order, bottom_up, mean, std, scale, bias, results,
                                  dict(color=color, post=post, warp=warp, tone=tone, enhance=enhance, alpha=alpha, resample=resample))

    @staticmethod
    def make_decode_batch_yuv(pngs, crops, outs, full, surface="nv12", depth=None, window=None, filter="bilinear", mirror=False, matrix=None, standard="bt709",
                              full_range=False):
        """Descriptor for decode_device_yuv() / decode_batch_yuv(): make_decode_batch_views() with surfaces in the place of the (c, h,
        w) views -- outs[i]: the list of file i's surfaces, each the tuple of plane tensors yuv_frame_layout() takes for `surface`,
        its Y plane (window h, window w).  crops, full, window, filter and mirror nest as there; surface, depth and the matrix (a (3, 4)
        one of the caller's, else yuv_matrix_from_rgb(standard, full_range)) are the call's."""
        fmt = _yuv_store_format("make_decode_batch_yuv", surface, depth, matrix, standard, full_range)
        outs = [[YuvSurface(t) for t in ts] for ts in outs]
        return _make_views_batch(_yuv_views(surface, fmt), pngs, crops, outs, full, window, filter, mirror, "rgb", False, None, None, None, None, {})

    def _decode_yuv(self, device_data, pngs, outs, surface, depth, crops, full, window, filter, mirror, matrix, standard, full_range, results):
        def make(who):
            cs, fs, dests = crops, full, outs
            if cs is None:  # (the whole of every file)
                cs = [[(0, 0) + _png_size(p)] for p in pngs]
            cs = [list(c) for c in cs]
            counts = [len(c) for c in cs]
            if fs is None:  # (every crop at its own size: the identity)
                fs = [[(int(c[2]), int(c[3])) for c in file] for file in cs]
            if dests is None or any(o is None for o in dests):  # (tight surfaces of each window's size)
                elems = {1: torch.uint8, 2: getattr(torch, "uint16", torch.int16)}
                fulls, windows = _per_view(who, counts, fs, "full sizes"), _per_view(who, counts, window, "windows")
                alloc = lambda hw: yuv_surface_planes(surface, hw[1], hw[0], lambda n, elem: torch.empty(n, dtype=elems[elem], device=f"cuda:{self.device}"))
                dests = [[alloc(_window_hw(f_, w_)) for f_, w_ in zip(fulls[i], windows[i])] if dests is None or dests[i] is None else dests[i] for i in range(len(cs))]
            return self.make_decode_batch_yuv(pngs, cs, dests, fs, surface, depth, window, filter, mirror, matrix, standard, full_range)

        return self._run_decode(DecodeBatchYuv, device_data, pngs, make, lambda b: views_entry("yuv", device_data, b), results)

    def decode_device_yuv(self, pngs, outs=None, surface="nv12", depth=None, crops=None, full=None, window=None, filter="bilinear", mirror=False, matrix=None,
                          standard="bt709", full_range=False, results=True):
        """fpng_amd_decode_batch_device_yuv_views: views of each file -- uint8 CUDA tensors holding whole files -- written as the YUV
        surfaces a hardware video encoder takes: "nv12", "p016" (depth 10 / 12 / 16: P010 / P012 / P016), "yuv444", "yuv444_16".
        Everything in front of the surface is decode_device_views(): crops[i] lists file i's crops (None: the whole file, one view),
        each resized to its full size (None: its own, the identity) by its filter, its window mirrored where asked; nested lists
        give several views per file from one decode of it -- one 4K file into 2160p, 1080p and 720p NV12 for an adaptive-bitrate
        ladder.  outs[i][k]: the surface of view k of file i, the tuple of plane tensors yuv_frame_layout() takes (any pitch, chroma
        anywhere); outs=None (or None for a file) allocates tight surfaces.  The rule (include/fpng_amd.h; yuv_surface() is its
        host twin): Y, Cb, Cr = the matrix's rows over R, G, B in fp32 fused multiply-adds, scaled to the depth, clamped and rounded
        to nearest even; 4:2:0 chroma from the MEAN of each 2 x 2 block (centre siting, no siting option).  matrix: a (3, 4) matrix of
        the caller's, else yuv_matrix_from_rgb(standard, full_range).  -> list, per file, of (status, the list of its surfaces or
        None, channels_in_file); results=False returns the descriptor.  pngs may be a make_decode_batch_yuv() descriptor."""
        return self._decode_yuv(True, pngs, outs, surface, depth, crops, full, window, filter, mirror, matrix, standard, full_range, results)

    def decode_batch_yuv(self, pngs, outs=None, surface="nv12", depth=None, crops=None, full=None, window=None, filter="bilinear", mirror=False, matrix=None,
                         standard="bt709", full_range=False, results=True):
        """fpng_amd_decode_batch_yuv_views: decode_device_yuv() for files in host memory (bytes)."""
        return self._decode_yuv(False, pngs, outs, surface, depth, crops, full, window, filter, mirror, matrix, standard, full_range, results)

    @staticmethod
    def make_decode_batch_views_hwc(pngs, crops, outs, full, window=None, filter="bilinear", mirror=False, order="rgb", bottom_up=False, mean=None, std=None,
                                    scale=None, bias=None, color=None, post=None, warp=None, tone=None, enhance=None, alpha=None, resample=None):
        """Descriptor for decode_device_views_hwc() / decode_batch_views_hwc(): make_decode_batch_views() with CHANNELS-LAST
        destinations -- outs[i] lists file i's (window h, window w, c) views (dest_layout_hwc() has their rules), all of one c per
        file and one dtype per call; the records are fpng_amd_view_dest_hwc.  Everything else -- the nesting of crops and outs, one
        value / per file / per view for full, window, filter, mirror, order and bottom_up, the constants, color (then:
        fpng_amd_decode_batch(_device)_hwc_views_color), post (then: fpng_amd_decode_batch(_device)_hwc_views_post), warp (then:
        fpng_amd_decode_batch(_device)_hwc_views_warp), tone (then: fpng_amd_decode_batch(_device)_hwc_views_tone), enhance (then:
        fpng_amd_decode_batch(_device)_hwc_views_enhance) alpha (then: fpng_amd_decode_batch(_device)_hwc_views_alpha) and resample
        (then: fpng_amd_decode_batch(_device)_hwc_views_resample) -- is make_decode_batch_views()'s."""
        return _make_views_batch(_HWC_VIEWS, pngs, crops, outs, full, window, filter, mirror, order, bottom_up, mean, std, scale, bias,
                                 dict(color=color, post=post, warp=warp, tone=tone, enhance=enhance, alpha=alpha, resample=resample))

    def decode_device_views_hwc(self, pngs, crops=None, outs=None, full=None, window=None, filter="bilinear", mirror=False, dtype=torch.uint8, order="rgb",
                                bottom_up=False, mean=None, std=None, scale=None, bias=None, results=True, color=None, post=None, warp=None, tone=None, enhance=None, alpha=None, resample=None):
        """fpng_amd_decode_batch_device_hwc_views: decode_device_views() into CHANNELS-LAST destinations -- each view's window is
        written to an (h, w, c) device tensor view, element (q, i, c) exactly what decode_device_views() writes at (c, q, i),
        without a permute copy.  For a batch that trains in torch.channels_last,

            x = torch.empty((n, 3, 224, 224), dtype=torch.float16, device="cuda", memory_format=torch.channels_last)

        file i's destination is x[i].permute(1, 2, 0); x stays contiguous in channels_last.  Also: a contiguous HWC tensor, a crop
        of one, rgba[..., :3] (the fourth element of every pixel is left alone), order "bgr" / "abgr", bottom_up
        (dest_layout_hwc() has the rules).  full equal to a crop's size with the whole window is the identity: a plain HWC crop,
        uint8 or float.  -> list, per file, of (status, the list of the caller's views or None, channels_in_file).  outs=None (or
        None for a file) allocates contiguous (h, w, 3) tensors of `dtype`.  pngs may be a make_decode_batch_views_hwc() descriptor
        of device files; results=False returns it.  color: as decode_device_views()'s (fpng_amd_decode_batch_device_hwc_views_color)."""
        return self._decode_views(_HWC_VIEWS, True, pngs, crops, outs, full, window, filter, mirror, dtype, order, bottom_up, mean, std, scale, bias, results,
                                  dict(color=color, post=post, warp=warp, tone=tone, enhance=enhance, alpha=alpha, resample=resample))

    def decode_batch_views_hwc(self, pngs, crops=None, outs=None, full=None, window=None, filter="bilinear", mirror=False, dtype=torch.uint8, order="rgb",
                               bottom_up=False, mean=None, std=None, scale=None, bias=None, results=True, color=None, post=None, warp=None, tone=None, enhance=None, alpha=None, resample=None):
        """fpng_amd_decode_batch_hwc_views: decode_device_views_hwc() for files in host memory (bytes)."""
        return self._decode_views(_HWC_VIEWS, False, pngs, crops, outs, full, window, filter, mirror, dtype, order, bottom_up, mean, std, scale, bias, results,
                                  dict(color=color, post=post, warp=warp, tone=tone, enhance=enhance, alpha=alpha, resample=resample))

    @staticmethod
    def make_decode_batch_png_views(pngs, crops, outs, full, window=None, filter="bilinear", mirror=False, order="rgb", bottom_up=False, mean=None, std=None,
                                    scale=None, bias=None, color=None, post=None, warp=None, tone=None, enhance=None, alpha=None, resample=None, layout="planar", flags=0):
        """Descriptor for decode_device_png_views() / decode_batch_png_views(): make_decode_batch_views() (layout="planar": (c, h, w)
        destinations) or make_decode_batch_views_hwc() (layout="hwc": (h, w, c) ones) for ORDINARY PNG files -- the same nesting of
        crops and outs, the same constants and the same stage keywords; flags: the call's (FPNG_AMD_PNG_GENERAL_ONLY)."""
        if layout not in _PNG_VIEWS:
            raise ValueError(f"make_decode_batch_png_views: layout {layout!r} (\"planar\" or \"hwc\")")
        batch = _make_views_batch(_PNG_VIEWS[layout], pngs, crops, outs, full, window, filter, mirror, order, bottom_up, mean, std, scale, bias,
                                  dict(color=color, post=post, warp=warp, tone=tone, enhance=enhance, alpha=alpha, resample=resample))
        batch.flags = int(flags)
        return batch

    def _decode_png_views(self, device_data, pngs, crops, outs, full, window, filter, mirror, dtype, order, bottom_up, mean, std, scale, bias, results, stages, layout, flags):
        if isinstance(pngs, DecodeBatchPngViews):  # (a descriptor knows its layout and carries its flags)
            layout, flags = ("hwc" if isinstance(pngs, DecodeBatchPngViewsHwc) else "planar"), pngs.flags
        if layout not in _PNG_VIEWS:
            raise ValueError(f"{DecodeBatchPngViews.call(device_data)}: layout {layout!r} (\"planar\" or \"hwc\")")
        lay = _PNG_VIEWS[layout]
        if isinstance(pngs, lay.batch_cls) and any(v is not None for v in stages.values()):
            raise ValueError(f"{lay.batch_cls.call(device_data)}: a descriptor carries its own records of the stages {', '.join(k for k, _, _, _ in _VIEW_STAGES)}")

        def make(who):
            dests = outs
            if crops is None or full is None:
                raise ValueError(f"{who}: crops, a list of (x, y, w, h) per file, and full, the (full_w, full_h) they are resized to")
            if outs is None or any(o is None for o in outs):  # (each window's size with c = 3; files with alpha lose it)
                where = dict(dtype=_alloc_dtype(who, dtype), device=f"cuda:{self.device}")
                counts = [len(c) for c in crops]
                fulls, windows = _per_view(who, counts, full, "full sizes"), _per_view(who, counts, window, "windows")
                dests = [[torch.empty(lay.empty_shape(*_window_hw(f_, w_)), **where) for f_, w_ in zip(fulls[i], windows[i])] if outs is None or outs[i] is None else outs[i]
                         for i in range(len(crops))]
            batch = _make_views_batch(lay, pngs, crops, dests, full, window, filter, mirror, order, bottom_up, mean, std, scale, bias, stages)
            batch.flags = int(flags)
            return batch

        return self._run_decode(lay.batch_cls, device_data, pngs, make, lambda b: png_views_entry(layout, device_data, b, b.flags), results)

    def decode_device_png_views(self, pngs, crops=None, outs=None, full=None, window=None, filter="bilinear", mirror=False, dtype=torch.uint8, order="rgb",
                                bottom_up=False, mean=None, std=None, scale=None, bias=None, results=True, color=None, post=None, warp=None, tone=None, enhance=None,
                                alpha=None, resample=None, layout="planar", flags=0):
        """fpng_amd_decode_batch_device_png_views: decode_device_views() (layout="planar") or decode_device_views_hwc()
        (layout="hwc") for ORDINARY PNG files -- what libpng, Pillow or zlib write: 8-bit grey, grey + alpha, RGB, palette, RGBA, not
        interlaced -- in uint8 CUDA tensors.  Every argument is the views call's, every stage keyword included; a view holds exactly
        what that call writes for an fpng-written file with the same pixels.  A file has an alpha plane, which the alpha records act
        on and a 4-channel destination gets, when decode_device_png() at 4 channels can give it an alpha below 255 (grey + alpha,
        RGBA, palette with tRNS, grey or RGB with a colour key); another file's fourth plane is 255.  Files with fpng's marker go
        through the fpng tier's views path unless flags has FPNG_AMD_PNG_GENERAL_ONLY.  -> list, per file, of (status, the list of
        the caller's views or None, channels_in_file): the statuses of decode_device_png(), a bad filter byte or palette index
        counting only where the file's one source box (views_source()) makes the decoder look, and
        FPNG_AMD_DECODE_PNG_CROP_OUTSIDE (68) for a crop that leaves the image -- 67 is FPNG_AMD_DECODE_UNSUPPORTED_PNG here.
        pngs may be a make_decode_batch_png_views() descriptor of device files; results=False returns it."""
        return self._decode_png_views(True, pngs, crops, outs, full, window, filter, mirror, dtype, order, bottom_up, mean, std, scale, bias, results,
                                      dict(color=color, post=post, warp=warp, tone=tone, enhance=enhance, alpha=alpha, resample=resample), layout, flags)

    def decode_batch_png_views(self, pngs, crops=None, outs=None, full=None, window=None, filter="bilinear", mirror=False, dtype=torch.uint8, order="rgb",
                               bottom_up=False, mean=None, std=None, scale=None, bias=None, results=True, color=None, post=None, warp=None, tone=None, enhance=None,
                               alpha=None, resample=None, layout="planar", flags=0):
        """fpng_amd_decode_batch_png_views: decode_device_png_views() for files in host memory (bytes)."""
        return self._decode_png_views(False, pngs, crops, outs, full, window, filter, mirror, dtype, order, bottom_up, mean, std, scale, bias, results,
                                      dict(color=color, post=post, warp=warp, tone=tone, enhance=enhance, alpha=alpha, resample=resample), layout, flags)

    def set_decode_verify(self, flags):
        """fpng_amd_encoder_set_decode_verify: every later decode call of this encoder also checks the files' IDAT CRC-32
        (VERIFY_CRC32) and / or the zlib stream's Adler-32 (VERIFY_ADLER32); 0 = neither (the default, and the reference's
        behaviour).  A file that would have decoded with status 0 then returns DECODE_BAD_CRC32 (65) or DECODE_BAD_ADLER32 (66)
        when the checksum in the file is not the one of its bytes; every other status stays what it is."""
        check(self.lib.fpng_amd_encoder_set_decode_verify(self.h, int(flags)))

    @property
    def decode_verify(self):
        return int(self.lib.fpng_amd_encoder_decode_verify(self.h))

    def last_decode_phase_ms(self):
        """{"sync", "offsets", "emit", "unfilter"} -> ms of the last decode call's kernels (first group of files), measured with HIP
        events on the encoder's stream while set_profiling(True)."""
        ms = (C.c_float * 4)()
        check(self.lib.fpng_amd_decode_last_phase_ms(self.h, C.byref(ms)))
        return dict(zip(("sync", "offsets", "emit", "unfilter"), (float(v) for v in ms)))

    def decode_host(self, png, desired_chans):
        """fpng_amd_decode_host: ONE fpng-written file (bytes) -> (status, uint8 numpy array (h, w, desired_chans) or None, channels_in_file);
        container checks, upload, GPU decode and one download into host memory (what fpng::fpng_decode_memory does for large images).
        status 64 (FPNG_AMD_DECODE_UNDECIDED): decode that file on the CPU."""
        b = np.frombuffer(bytes(png), dtype=np.uint8)
        res = _lib.DecodeResult()
        hold = []

        def reserve(_user, nbytes):
            hold[:] = [np.empty(nbytes, dtype=np.uint8)]
            return hold[0].ctypes.data

        cb = _lib.RESERVE_FN(reserve)
        self._sync_stream()
        check(self.lib.fpng_amd_decode_host(self.h, b.ctypes.data if b.size else None, b.size, desired_chans, cb, None, C.byref(res)))
        if res.status or not hold:
            return res.status, None, res.channels_in_file
        return 0, hold[0].reshape(res.h, res.w, desired_chans), res.channels_in_file

    def train_tables(self, images):
        """fpng_amd_train_tables: a new 1-pass table from a corpus of uint8 CUDA tensors (h, w, c), all with the same c, in the
        form the reference's training mode prints it (block prefix bytes as hex, pending bits, codes, code sizes)."""
        n = len(images)
        c = images[0].shape[2]
        arr = (Image * n)()
        for i, im in enumerate(images):
            assert im.is_cuda and im.dtype == torch.uint8 and im.is_contiguous() and im.dim() == 3
            arr[i].d_pixels = im.data_ptr()
            arr[i].w, arr[i].h, arr[i].num_chans = im.shape[1], im.shape[0], im.shape[2]
        prefix = (C.c_uint8 * 512)()
        nb, bb, bbs = C.c_size_t(0), C.c_uint32(0), C.c_uint32(0)
        codes = (C.c_uint32 * 288)()
        sizes = (C.c_uint8 * 288)()
        self._sync_stream()
        check(self.lib.fpng_amd_train_tables(self.h, arr, n, c, prefix, 512, C.byref(nb), C.byref(bb), C.byref(bbs), codes, sizes))
        return {"prefix": bytes(prefix[: nb.value]).hex(), "bit_buf": bb.value, "bit_buf_size": bbs.value, "codes": list(codes),
                "code_sizes": list(sizes)}

    # ---- host buffers: what fpng_encode_image_to_memory() does ----
    def encode_host(self, image, w, h, num_chans, flags=0):
        b = _as_u8(image)
        if b.size < w * h * num_chans:
            raise ValueError("image buffer smaller than w*h*num_chans")
        cap = max_encoded_size(w, h, num_chans) if (w and h and num_chans in (3, 4)) else 64
        out = np.empty(cap, dtype=np.uint8)
        n = C.c_size_t(0)
        self._sync_stream()
        check(self.lib.fpng_amd_encode_host(self.h, b.ctypes.data, w, h, num_chans, flags, out.ctypes.data, cap,
                                            C.byref(n)))
        return out[: n.value].tobytes()

    def encode_host_into(self, image, w, h, num_chans, out, flags=0):
        """Like encode_host() but into a caller-owned uint8 numpy array (>= max_encoded_size bytes), returning the
        PNG size: no allocation and no copy on the Python side, so a capture loop can reuse its buffers
        (3.6 ms instead of 18 ms per 8K frame: the one-shot form pays for a fresh 133 MB array and a bytes copy)."""
        b = _as_u8(image)
        if b.size < w * h * num_chans:
            raise ValueError("image buffer smaller than w*h*num_chans")
        assert out.dtype == np.uint8 and out.flags["C_CONTIGUOUS"]
        n = C.c_size_t(0)
        self._sync_stream()
        check(self.lib.fpng_amd_encode_host(self.h, b.ctypes.data, w, h, num_chans, flags, out.ctypes.data, out.size,
                                            C.byref(n)))
        return n.value

    def last_host_bands(self):
        """Row bands the last encode_host*() call was streamed in (1 = upload, encode, download one after the other)."""
        return self.lib.fpng_amd_encoder_last_host_bands(self.h)

    def encode_host_batch(self, images, flags=0, outs=None, paths=None, writer_threads=0):
        """Many host frames (uint8 arrays shaped (h, w, c)): uploads, encodes, downloads and file writes of consecutive
        frames overlap (fpng_amd_encode_host_batch).  outs: caller-owned uint8 arrays (>= max_encoded_size) or None when
        every frame goes to a file; paths: file names or None.  Returns the PNG sizes."""
        arr, sizes, keep = _host_batch_records(images, outs, paths)
        check(self.lib.fpng_amd_encode_host_batch(self.h, arr, len(images), flags, writer_threads))
        return [int(s) for s in sizes]

    def encode_host_growing(self, image, w, h, num_chans, flags=0):
        """fpng_amd_encode_host_to() with a growing bytearray as the output allocator (what the fpng:: drop-in does with
        its std::vector): returns (png bytes, list of the sizes the encoder asked for)."""
        b = _as_u8(image)
        buf = bytearray()
        asked = []
        hold = []

        def reserve(_user, nbytes):
            asked.append(nbytes)
            hold[:] = []  # (a bytearray cannot grow while a ctypes view of it is alive)
            if len(buf) < nbytes:
                buf.extend(bytes(nbytes - len(buf)))
            hold[:] = [(C.c_uint8 * len(buf)).from_buffer(buf)]
            return C.addressof(hold[0])

        cb = _lib.RESERVE_FN(reserve)
        n = C.c_size_t(0)
        self._sync_stream()
        rc = self.lib.fpng_amd_encode_host_to(self.h, b.ctypes.data, w, h, num_chans, flags, cb, None, C.byref(n))
        hold[:] = []
        check(rc)
        return bytes(buf[: n.value]), asked

    # ---- row bands (multi-GPU, one image): see include/fpng_amd.h ----
    @staticmethod
    def _band(rows, row_above, w, num_chans, y0, y1, h_total):
        for t in (rows, row_above):
            if t is not None:
                assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous(), "band rows must be contiguous uint8 CUDA tensors"
        b = Band()
        b.d_rows = rows.data_ptr()
        b.d_row_above = row_above.data_ptr() if row_above is not None else None
        b.w, b.num_chans, b.y0, b.y1, b.h_total = w, num_chans, y0, y1, h_total
        return b

    def band_hist(self, band, d_hist):
        self._sync_stream()
        check(self.lib.fpng_amd_band_hist(self.h, C.byref(band), d_hist.data_ptr()))

    def band_encode(self, band, flags=0, d_hist=None):
        self._sync_stream()
        st = BandStats()
        check(self.lib.fpng_amd_band_encode(self.h, C.byref(band), flags, d_hist.data_ptr() if d_hist is not None else None, C.byref(st)))
        return st

    def band_place(self, band, start_bit, zlib_size, window):
        off, n = C.c_uint64(0), C.c_size_t(0)
        self._sync_stream()
        check(self.lib.fpng_amd_band_place(self.h, C.byref(band), start_bit, zlib_size, window.data_ptr(), window.numel(),
                                           C.byref(off), C.byref(n)))
        return off.value, n.value

    def band_crc_partials(self, device):
        """CRC partials (one uint32 per 64 KiB range of the file, as an int32 tensor) of the band placed last: XOR the
        ranks' arrays and hand the result to wrap_png()."""
        n = C.c_uint32(0)
        self._sync_stream()
        check(self.lib.fpng_amd_band_crc_partials(self.h, None, 0, C.byref(n)))  # (asks for the count)
        t = torch.empty(n.value, dtype=torch.int32, device=device)
        check(self.lib.fpng_amd_band_crc_partials(self.h, t.data_ptr(), n.value, C.byref(n)))
        return t

    def wrap_png(self, png_buf, zlib_size, adler, w, h, num_chans, crc_partials=None):
        n = C.c_size_t(0)
        self._sync_stream()
        if crc_partials is None:
            check(self.lib.fpng_amd_wrap_png(self.h, png_buf.data_ptr(), zlib_size, adler, w, h, num_chans, C.byref(n)))
        else:
            crc_partials = crc_partials.contiguous()
            self._keep_partials = crc_partials  # (asynchronous: keep it alive until the next call)
            check(self.lib.fpng_amd_wrap_png_crc(self.h, png_buf.data_ptr(), zlib_size, adler, w, h, num_chans,
                                                 crc_partials.data_ptr(), crc_partials.numel(), C.byref(n)))
        return n.value

    # ---- instrumentation ----
    def set_profiling(self, on=True):
        check(self.lib.fpng_amd_encoder_set_profiling(self.h, int(on)))

    def last_phase_ms(self):
        arr = (C.c_float * _lib.NUM_PHASES)()
        check(self.lib.fpng_amd_encoder_last_phase_ms(self.h, C.byref(arr)))
        return list(arr)


_default_encoder = None


def _encoder():
    global _default_encoder
    if _default_encoder is None:
        _default_encoder = Encoder(device=torch.cuda.current_device() if torch.cuda.is_available() else 0)
    return _default_encoder


def fpng_encode_image_to_memory(image, w, h, num_chans, flags=0):
    """Reference src/fpng.h:48.  Returns (ok, png_bytes); ok is False exactly where the reference
    returns false (bad dimensions / channel count, src/fpng.cpp:1670-1680).  Everything else
    (missing GPU, HIP errors) raises: it is not silently papered over."""
    try:
        return True, _encoder().encode_host(image, w, h, num_chans, flags)
    except FpngAmdError as e:
        if e.code == -1:  # FPNG_AMD_ERR_INVALID_ARG
            return False, b""
        raise


def fpng_encode_image_to_file(filename, image, w, h, num_chans, flags=0):
    """Reference src/fpng.h:52 / src/fpng.cpp:1806-1828."""
    ok, png = fpng_encode_image_to_memory(image, w, h, num_chans, flags)
    if not ok:
        return False
    try:
        with open(filename, "wb") as f:
            f.write(png)
    except OSError:
        return False
    return True

