"""The sweep of scale ratios that test_gpu_decode_views_ratios.py decodes and test_views_ratio_sweep_cpu.py keeps honest: one
3-channel 128 x 128 image, and per filter one view per (in, out) pair of INS x OUTS inside the filter's limit -- pair k on the
view's x axis, pair n - 1 - k on its y axis, a crop whose origin moves with k, no window, the mirror flag alternating.  No library
and no GPU in here: sizes, the image and the model's bytes (resample_model / resize_view_model)."""
import numpy as np

import resample_model as SM  # (before any model is asked for a new filter's name)
import resize_view_model as VM

SIZE = 128
INS = list(range(1, 65)) + [96, 127, 128]
OUTS = list(range(1, 25)) + [33, 64]
FILTERS = SM.NEW_FILTERS + VM.FILTERS
PAIRS = {"nearest": 1702, "box": 1702, "hamming": 1702, "bilinear": 1702, "lanczos": 1550, "bicubic": 1627}


def image(rows=SIZE):
    """(rows, SIZE, 3) uint8 noise whose even columns and even rows are 0 or 255: the sums of both passes reach both clips"""
    rng = np.random.default_rng(2026)
    px = rng.integers(0, 256, (SIZE, SIZE, 3), dtype=np.uint8)
    ends = rng.choice(np.array([0, 255], dtype=np.uint8), px.shape)
    px[::2, :] = ends[::2, :]
    px[:, ::2] = ends[:, ::2]
    return np.ascontiguousarray(px[:rows])


def pairs(filter):
    return [(i, o) for i in INS for o in OUTS if SM.scale_ok(i, o, filter)]


def views(filter):
    """[(crop, full, mirror)] of the filter's views, in the call's order"""
    ps = pairs(filter)
    out = []
    for k, (ix, ox) in enumerate(ps):
        iy, oy = ps[len(ps) - 1 - k]
        out.append(((7 * k % (SIZE - ix + 1), 13 * k % (SIZE - iy + 1), ix, iy), (ox, oy), bool(k & 1)))
    return out


def expected(planes, filter, only=None):
    """the model's (3, out_y, out_x) uint8 planes of every view (of the views `only`: a set of indices; None elsewhere), not
    mirrored, from the image's (3 or 4, SIZE, SIZE) planes"""
    return [VM.view_planes(planes[:3, y:y + h, x:x + w], full, None, filter) if only is None or k in only else None for k, ((x, y, w, h), full, _) in enumerate(views(filter))]
