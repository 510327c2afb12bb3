"""The rule of fpng_amd_decode_batch(_device)_planar_resize_view, restated in Python on top of
resize_model.py: Pillow's 8-bit resampler with a choice of filter -- "bilinear" (the triangle, support 1: resize_model's own weights)
or "bicubic" (the Keys cubic with a = -0.5, support 2) -- and a window of the resized image, which is a slice of it.  Weights in
plain Python floats (IEEE double, one operation at a time, in the order the rule writes them), passes in integers.
test_resize_view_cpu.py pins this text to Pillow and the library's fpng_amd_resize_weights_filter / fpng_amd_resize_view_source to
this text; the GPU tests take their expected bytes from here."""
import functools

import numpy as np

import resize_model as RM

PRECISION_BITS = RM.PRECISION_BITS
MAX_TAPS = RM.MAX_TAPS
MAX_SCALE = {"bilinear": 32, "bicubic": 16}  # in <= MAX_SCALE * out
SUPPORT = {"bilinear": 1.0, "bicubic": 2.0}
FILTERS = ("bilinear", "bicubic")


def _cubic(a):
    x = abs(a)
    if x < 1.0:
        return ((1.5 * x - 2.5) * x) * x + 1.0
    if x < 2.0:
        return (((x - 5.0) * x + 8.0) * x - 4.0) * -0.5
    return 0.0


KERNEL = {"bilinear": RM._tri, "bicubic": _cubic}


def _fixed(v):
    return int(-0.5 + v * 4194304.0) if v < 0.0 else int(0.5 + v * 4194304.0)  # int(): truncation toward zero


@functools.lru_cache(maxsize=None)
def axis_weights(in_size, out_size, filter="bilinear"):
    """(first[out], count[out], K[out][count]) of one axis: Python ints"""
    kf = KERNEL[filter]
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = SUPPORT[filter] * fs
    ss = 1.0 / fs
    firsts, counts, weights = [], [], []
    for o in range(out_size):
        center = (o + 0.5) * scale
        first = max(int(center - support + 0.5), 0)
        count = min(int(center + support + 0.5), in_size) - first
        k = [kf(((t + first) - center + 0.5) * ss) for t in range(count)]
        ww = 0.0
        for v in k:
            ww += v
        if ww != 0.0:
            k = [v / ww for v in k]
        firsts.append(first)
        counts.append(count)
        weights.append([_fixed(v) for v in k])
    return firsts, counts, weights


def one_pass_sums(rows, out_size, filter):
    """rows (m, in) uint8 -> (m, out) int64: the pass's sums before the shift and the clamp"""
    rows = np.asarray(rows, dtype=np.uint8)
    first, count, K = axis_weights(rows.shape[1], out_size, filter)
    out = np.empty((rows.shape[0], out_size), dtype=np.int64)
    wide = rows.astype(np.int64)
    for o in range(out_size):
        out[:, o] = wide[:, first[o]:first[o] + count[o]] @ np.asarray(K[o], dtype=np.int64) + (1 << (PRECISION_BITS - 1))
    return out


def one_pass(rows, out_size, filter):
    """rows (m, in) uint8 -> (m, out) uint8: the pass along the last axis (>>: numpy's arithmetic shift, floor)"""
    return np.clip(one_pass_sums(rows, out_size, filter) >> PRECISION_BITS, 0, 255).astype(np.uint8)


def resize_plane(p, full_w, full_h, filter="bilinear"):
    """p (h, w) uint8 -> (full_h, full_w) uint8: the horizontal pass to clamped bytes, then the vertical pass to clamped bytes"""
    t = one_pass(p, full_w, filter)
    return np.ascontiguousarray(one_pass(np.ascontiguousarray(t.T), full_h, filter).T)


def view_planes(px, full, window=None, filter="bilinear", mirror=False):
    """px (c, h, w) uint8, the crop's planes -> (c, window h, window w) uint8: every plane resized WHOLE to full = (full_w, full_h)
    and sliced to window = (x, y, w, h) (None: all of it); mirror: the window's columns in reverse order"""
    x, y, w, h = (0, 0, full[0], full[1]) if window is None else window
    r = np.stack([resize_plane(px[c], full[0], full[1], filter)[y:y + h, x:x + w] for c in range(px.shape[0])])
    return np.ascontiguousarray(r[:, :, ::-1]) if mirror else np.ascontiguousarray(r)


def axis_span(in_size, out_size, o0, n, filter):
    """(begin, end) of the source samples that output samples o0 .. o0 + n - 1 have taps at"""
    first, count, _ = axis_weights(in_size, out_size, filter)
    return first[o0], first[o0 + n - 1] + count[o0 + n - 1]


def view_source(crop, full, window=None, filter="bilinear"):
    """the box (x, y, w, h), in the file's coordinates, of the source pixels that the window's taps reach"""
    x, y, w, h = (0, 0, full[0], full[1]) if window is None else window
    x0, x1 = axis_span(crop[2], full[0], x, w, filter)
    y0, y1 = axis_span(crop[3], full[1], y, h, filter)
    return crop[0] + x0, crop[1] + y0, x1 - x0, y1 - y0


# ---- the views test_gpu_resize_view.py decodes (test_resize_view_cpu.py judges fpng_amd_resize_view_source on them too):
#      file (w, h) -> [(crop, full, window or None, filters)] ----
BOTH = FILTERS
VIEWS = {
    (600, 130): [
        ((0, 0, 600, 130), (224, 224), None, BOTH),                 # shrink in x, grow in y; bilinear: the plain resize call's bytes
        ((0, 0, 600, 130), (256, 256), (16, 16, 224, 224), BOTH),   # the evaluation shape
        ((0, 0, 600, 130), (300, 65), (235, 48, 65, 17), BOTH),     # the far corner: taps clipped right and below, one past a tile
        ((0, 0, 600, 130), (300, 65), (140, 30, 20, 10), BOTH),     # a box past the first 256-column block and 48-row segment
        ((5, 7, 9, 11), (65, 17), None, BOTH),                      # an upscale
        ((250, 40, 13, 20), (13, 20), None, BOTH),                  # the identity across a tile border of the pixel pass
        ((0, 0, 96, 64), (6, 4), None, ("bicubic",)),               # exactly 16 x
        ((0, 0, 96, 64), (3, 2), None, ("bilinear",)),              # exactly 32 x
        ((0, 0, 600, 130), (224, 224), (0, 0, 1, 1), BOTH),         # 1 x 1 windows at both ends
        ((0, 0, 600, 130), (224, 224), (223, 223, 1, 1), BOTH),
    ],
    (257, 49): [((0, 0, 257, 49), (129, 25), (64, 16, 64, 9), BOTH)],
    (64, 97): [((0, 0, 64, 97), (128, 194), (63, 0, 2, 194), BOTH)],
    (1, 1): [((0, 0, 1, 1), (5, 5), (2, 2, 3, 3), BOTH)],
}
