"""The rule of fpng_amd_decode_batch(_device)_yuv_views (include/fpng_amd.h, csrc/yuv_store.h) in numpy, without the library:

    t_c(r, g, b) = fmaf(f[c][2], b, fmaf(f[c][1], g, fmaf(f[c][0], r, f[c][3])))       c = Y, Cb, Cr
    elem_d(t)    = rint(min(max(t * 2^(d-8), 0), 2^d - 1)), ties to even
    Y = elem_d(t_0(pixel));  4:4:4: Cb, Cr = elem_d(t_1(pixel)), elem_d(t_2(pixel))
    4:2:0: S_k = the integer sum of plane k over the 2 x 2 block, a missing column or row counted twice;  m_k = S_k * 0.25
           Cb, Cr = elem_d(t_1(m)), elem_d(t_2(m))
    a 16-bit element is stored as elem_d << (16 - d)

The arithmetic is color_model.fma32_np's (one rounding per fmaf), the block sums are slices of an edge-padded integer array, so no
element needs a tolerance.  The matrix construction of fpng_amd_yuv_matrix_from_rgb is recomputed here; surface layouts are
yuv_model.Layout's."""
import numpy as np

from color_model import fma32_np
from yuv_model import KR_KB, Layout, SURFACES, elem_bytes, is_420  # noqa: F401  (re-exported for the tests)

DEPTHS = {"nv12": (8,), "yuv444": (8,), "p016": (10, 12, 16), "yuv444_16": (10, 12, 16)}
CASES = [(s, d) for s in SURFACES for d in DEPTHS[s]]


def matrix(standard, full_range):
    """fpng_amd_yuv_matrix_from_rgb's construction: every coefficient in double from Kr and Kb, rounded to fp32"""
    kr, kb = KR_KB[standard]
    kg = 1.0 - kr - kb
    sy, sc, y0 = (1.0, 1.0, 0.0) if full_range else (219.0 / 255.0, 224.0 / 255.0, 16.0)
    coef = [[kr * sy, kg * sy, kb * sy, y0],
            [-kr / (2.0 * (1.0 - kb)) * sc, -kg / (2.0 * (1.0 - kb)) * sc, 0.5 * sc, 128.0],
            [0.5 * sc, -kg / (2.0 * (1.0 - kr)) * sc, -kb / (2.0 * (1.0 - kr)) * sc, 128.0]]
    return np.asarray(coef, dtype=np.float64).astype(np.float32)


def _elem(t, d):
    t = t * np.float32(2.0 ** (d - 8))  # (exact: a power of two, far from overflow)
    return np.rint(np.minimum(np.maximum(t, np.float32(0.0)), np.float32(2 ** d - 1))).astype(np.uint32)


def _mix(m, c, r, g, b):
    return fma32_np(m[c, 2], b, fma32_np(m[c, 1], g, fma32_np(m[c, 0], r, m[c, 3])))


def block_sums(plane):
    """(ceil(h / 2), ceil(w / 2)) integer sums of a plane's 2 x 2 blocks: at an odd edge the existing pixels count twice"""
    h, w = plane.shape
    p = np.pad(plane.astype(np.int64), ((0, h & 1), (0, w & 1)), mode="edge")
    return p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2]


def surface(rgb, surf, depth, m):
    """rgb (h, w, 3) uint8 -> the surface's planes as yuv_frame_layout takes them: Y (h, w) and CbCr (ceil(h / 2), ceil(w / 2), 2),
    or Y, Cb, Cr, each (h, w); uint8, or uint16 words with the element MSB-aligned"""
    m = np.asarray(m, dtype=np.float32)
    rgb = np.asarray(rgb, dtype=np.uint8)
    ch = [rgb[..., k].astype(np.float32) for k in range(3)]
    e = elem_bytes(surf)
    dt, shift = (np.uint16, 16 - depth) if e == 2 else (np.uint8, 0)
    put = lambda v: (v << shift).astype(dt)
    y = put(_elem(_mix(m, 0, *ch), depth))
    if not is_420(surf):
        return y, put(_elem(_mix(m, 1, *ch), depth)), put(_elem(_mix(m, 2, *ch), depth))
    mean = [block_sums(rgb[..., k]).astype(np.float32) * np.float32(0.25) for k in range(3)]
    return y, np.stack([put(_elem(_mix(m, 1, *mean), depth)), put(_elem(_mix(m, 2, *mean), depth))], axis=-1)


def write(planes, views):
    """the model's planes into the views of a laid-out surface (yuv_model.Layout.numpy_views)"""
    for p, v in zip(planes, views):
        v[...] = p.view(v.dtype) if p.dtype.itemsize == v.dtype.itemsize else p


def corner_patch():
    """(12, 18, 3): the 216 colours with 0, 1, 127, 128, 254 or 255 in every channel, shuffled (a fixed order) so that the 2 x 2 blocks
    of every channel have sums of every residue mod 4 -- means that end in .0, .25, .5 and .75"""
    vals = np.array([0, 1, 127, 128, 254, 255], dtype=np.uint8)
    r, g, b = np.meshgrid(vals, vals, vals, indexing="ij")
    colours = np.stack([r, g, b], axis=-1).reshape(216, 3)
    return np.ascontiguousarray(colours[np.random.default_rng(216).permutation(216)].reshape(12, 18, 3))


def content(rng, w, h):
    """random bytes with the corner patch (as much of it as fits) in the top left corner"""
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    patch = corner_patch()[:h, :w]
    img[:patch.shape[0], :patch.shape[1]] = patch
    return img
