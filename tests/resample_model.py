"""The rules of the RESAMPLE record of fpng_amd_decode_batch(_device)_{planar,hwc}_views_resample,
restated in Python without the library: Pillow's "nearest", "box", "hamming" and "lanczos" filters next to resize_view_model's
"bilinear" and "bicubic".

box, hamming and lanczos are convolutions under resize_view_model's rule, unchanged -- centre, first, count, the two walks, the
division by ww, 2^22 fixed point -- each with a kernel function of the SIGNED argument and a base support:

    box(a)     = a > -0.5 and a <= 0.5 ? 1 : 0                                                      s_f = 0.5
    hamming(a) = x = |a|;  x == 0 ? 1 : x >= 1 ? 0 : (x = x * pi;  sin(x) / x * (C0 + C1 * cos(x)))  s_f = 1
                 C0, C1: 0.54 and 0.46 rounded to FLOAT and widened again (Pillow writes them 0.54f, 0.46f)
    lanczos(a) = -3 <= a < 3 ? sinc(a) * sinc(a / 3) : 0;  sinc(x) = x == 0 ? 1 : (x = x * pi;  sin(x) / x)    s_f = 3

with libm's sin and cos (math.sin, math.cos).  nearest is Pillow's affine scale path: per axis a = in / out, xo = a * 0.5, and for
o = 0 .. out - 1: idx[o] = int(xo), then xo += a -- the running sum is part of the rule.  In the passes it is one tap of weight
2^22 at idx[o]: (2^21 + v * 2^22) >> 22 = v.

Importing this module teaches resize_view_model the four names (its KERNEL, SUPPORT and MAX_SCALE tables and its axis_weights,
whose answers for "bilinear" and "bicubic" stay what they were; its FILTERS tuple is not touched), so every model built on it --
alpha_model, enhance_model and what they use -- takes filter="nearest" ... as it takes "bicubic".  test_views_resample_cpu.py pins
this text to Pillow and the library's host twins to this text; the GPU tests take their expected bytes from here."""
import functools
import math
import struct

import resize_view_model as VM

NEW_FILTERS = ("nearest", "box", "hamming", "lanczos")
RESAMPLE = {"nearest": 1, "box": 2, "hamming": 3, "lanczos": 4}  # FPNG_AMD_RESAMPLE_*


def _f32(v):
    return struct.unpack("f", struct.pack("f", v))[0]


_C0, _C1 = _f32(0.54), _f32(0.46)


def _box(a):
    return 1.0 if -0.5 < a <= 0.5 else 0.0


def _hamming(a):
    x = abs(a)
    if x == 0.0:
        return 1.0
    if x >= 1.0:
        return 0.0
    x = x * math.pi
    return math.sin(x) / x * (_C0 + _C1 * math.cos(x))


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(a):
    return _sinc(a) * _sinc(a / 3) if -3.0 <= a < 3.0 else 0.0


def scale_ok(in_size, out_size, filter):
    """the library's limit: in * max(s_f, 1) <= 32 * out"""
    return in_size >= 1 and out_size >= 1 and in_size * max(VM.SUPPORT[filter], 1.0) <= 32 * out_size


def nearest_indices(in_size, out_size):
    a = in_size / out_size
    xo = a * 0.5
    idx = []
    for _ in range(out_size):
        idx.append(int(xo))
        xo += a
    assert all(0 <= i < in_size for i in idx), (in_size, out_size)
    return idx


def product_indices(in_size, out_size):
    """what the rule is NOT: the index without the running sum"""
    a = in_size / out_size
    return [int((o + 0.5) * a) for o in range(out_size)]


_vm_axis_weights = VM.axis_weights


@functools.lru_cache(maxsize=None)
def axis_weights(in_size, out_size, filter="bilinear"):
    """(first[out], count[out], K[out][count]) of one axis, every filter"""
    if filter == "nearest":
        idx = nearest_indices(in_size, out_size)
        return idx, [1] * out_size, [[1 << VM.PRECISION_BITS] for _ in idx]
    return _vm_axis_weights(in_size, out_size, filter)


VM.KERNEL.update({"box": _box, "hamming": _hamming, "lanczos": _lanczos})
VM.SUPPORT.update({"nearest": 1.0, "box": 0.5, "hamming": 1.0, "lanczos": 3.0})  # (nearest: for scale_ok only)
VM.MAX_SCALE.update({"nearest": 32, "box": 32, "hamming": 32})  # lanczos: 3 * in <= 32 * out, no whole number
VM.axis_weights = axis_weights

view_planes = VM.view_planes
view_source = VM.view_source
resize_plane = VM.resize_plane

# ---- the views test_gpu_decode_views_resample.py decodes, after resize_view_model.VIEWS: file (w, h) -> [(crop, full, window or None,
#      filters)] ----
ALL = NEW_FILTERS
VIEWS = {
    (600, 130): [
        ((0, 0, 600, 130), (224, 224), None, ALL),                 # shrink in x, grow in y
        ((0, 0, 600, 130), (256, 256), (16, 16, 224, 224), ALL),   # the evaluation shape
        ((0, 0, 600, 130), (300, 65), (235, 48, 65, 17), ALL),     # the far corner: taps clipped right and below, one past a tile
        ((0, 0, 600, 130), (224, 224), (0, 0, 1, 1), ALL),         # 1 x 1 windows at both ends
        ((0, 0, 600, 130), (224, 224), (223, 223, 1, 1), ALL),
        ((5, 7, 9, 11), (65, 17), None, ALL),                      # an upscale
        ((250, 40, 13, 20), (13, 20), None, ALL),                  # the identity across a tile border of the pixel pass
        ((0, 0, 96, 64), (3, 2), None, ("nearest", "box", "hamming")),  # exactly 32 x
        ((0, 0, 96, 64), (9, 6), None, ("lanczos",)),              # exactly 3 * in = 32 * out
    ],
    (1, 1): [((0, 0, 1, 1), (5, 5), None, ALL)],
}
