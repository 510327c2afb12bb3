"""The resize rule of fpng_amd_decode_batch(_device)_planar_resize, restated in Python: Pillow's 8-bit
resampler with the triangle filter.  The weights are computed with plain Python floats (IEEE double, one operation at a time, in the
order the rule writes them); the passes are integer sums.  test_resize_cpu.py pins this text to Pillow itself and the library's
fpng_amd_resize_weights to this text; the GPU tests take their expected bytes from here."""
import functools

import numpy as np

PRECISION_BITS = 22
MAX_TAPS = 65   # count at the scale limit
MAX_SCALE = 32  # in <= 32 * out


def _tri(a):
    a = abs(a)
    return 1.0 - a if a < 1.0 else 0.0


@functools.lru_cache(maxsize=None)
def axis_weights(in_size, out_size):
    """(first[out], count[out], K[out][count]) of one axis: Python ints"""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = fs
    ss = 1.0 / fs
    firsts, counts, weights = [], [], []
    for o in range(out_size):
        center = (o + 0.5) * scale
        first = max(int(center - support + 0.5), 0)  # int(): truncation toward zero
        count = min(int(center + support + 0.5), in_size) - first
        k = [_tri(((t + first) - center + 0.5) * ss) for t in range(count)]
        ww = 0.0
        for v in k:
            ww += v
        if ww != 0.0:
            k = [v / ww for v in k]
        firsts.append(first)
        counts.append(count)
        weights.append([int(0.5 + v * 4194304.0) for v in k])
    return firsts, counts, weights


def one_pass(rows, out_size):
    """rows (m, in) uint8 -> (m, out) uint8: the pass along the last axis"""
    rows = np.asarray(rows, dtype=np.uint8)
    first, count, K = axis_weights(rows.shape[1], out_size)
    out = np.empty((rows.shape[0], out_size), dtype=np.uint8)
    wide = rows.astype(np.int64)
    for o in range(out_size):
        s = wide[:, first[o]:first[o] + count[o]] @ np.asarray(K[o], dtype=np.int64) + (1 << (PRECISION_BITS - 1))
        out[:, o] = np.clip(s >> PRECISION_BITS, 0, 255)
    return out


def resize_plane(p, out_w, out_h):
    """p (h, w) uint8 -> (out_h, out_w) uint8: the horizontal pass to bytes, then the vertical pass to bytes"""
    t = one_pass(p, out_w)
    return np.ascontiguousarray(one_pass(np.ascontiguousarray(t.T), out_h).T)


def resize_planes(px, out_w, out_h, mirror=False):
    """px (c, h, w) uint8 -> (c, out_h, out_w) uint8, every plane on its own; mirror: the columns in reverse order"""
    r = np.stack([resize_plane(px[c], out_w, out_h) for c in range(px.shape[0])])
    return np.ascontiguousarray(r[:, :, ::-1]) if mirror else r
