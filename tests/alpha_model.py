"""An exact restatement of the alpha rule of fpng_amd_decode_batch(_device)_planar_views_alpha / _hwc_views_alpha (include/fpng_amd.h,
INTEGRATION.md section 7) that does not use the library -- numpy integers throughout:

    M(v, a)    = t = v * a + 128;  ((t >> 8) + t) >> 8                       RGBA -> RGBa
    U(v, a)    = a == 0 or a == 255 ? v : min(255, (255 * v) // a)           RGBa -> RGBA
    C(v, a, b) = t = v * a + b * (255 - a) + 128;  ((t >> 8) + t) >> 8       over an opaque background

    composite:      P'_c = C(P_c, P_3, background[c]), P'_3 = 255;  R = the resize of P'
    premultiplied:  P'_c = M(P_c, P_3), P'_3 = P_3;  R' = the resize of P';  R_c = U(R'_c, R'_3), R_3 = R'_3

and of a whole view, which composes resize_view_model.py (the resize, per plane, on P') and enhance_model.view_elements (every later
stage, on R).  An alpha record here is a dict of fpng_amd.view_alpha()'s arguments: {} (no op), {"op": "composite", "background":
(r, g, b)} or {"op": "premultiplied"}.  test_views_alpha_cpu.py pins this text to Pillow and the library's host twins to this text;
the GPU tests take their expected bytes from here."""
import numpy as np

import enhance_model as EM
import resize_view_model as VM


def _wide(*arrays):
    return [np.asarray(a).astype(np.int64) for a in arrays]


def M(v, a):
    v, a = _wide(v, a)
    t = v * a + 128
    return (((t >> 8) + t) >> 8).astype(np.uint8)


def U(v, a):
    v, a = _wide(v, a)
    q = np.minimum(255, (255 * v) // np.where(a == 0, 1, a))
    return np.where((a == 0) | (a == 255), v, q).astype(np.uint8)


def C(v, a, b):
    v, a, b = _wide(v, a, b)
    t = v * a + b * (255 - a) + 128
    return (((t >> 8) + t) >> 8).astype(np.uint8)


def _op(alpha):
    op = (alpha or {}).get("op")
    assert op in (None, "composite", "premultiplied"), alpha
    return op


def source(alpha, px4):
    """step 1: (4, h, w) uint8 planes P -> P'"""
    px4 = np.asarray(px4, dtype=np.uint8)
    op = _op(alpha)
    if op == "composite":
        bg = alpha.get("background", (0, 0, 0))
        return np.stack([C(px4[c], px4[3], bg[c]) for c in range(3)] + [np.full_like(px4[3], 255)])
    if op == "premultiplied":
        return np.stack([M(px4[c], px4[3]) for c in range(3)] + [px4[3]])
    return px4.copy()


def result(alpha, r4):
    """step 3: (4, h, w) uint8 planes R' -> R"""
    r4 = np.asarray(r4, dtype=np.uint8)
    if _op(alpha) == "premultiplied":
        return np.stack([U(r4[c], r4[3]) for c in range(3)] + [r4[3]])
    return r4.copy()


def resized(alpha, px4, full, filter):
    """R' of the crop's planes px4 (4, h, w): P' resized WHOLE to full = (full_w, full_h), per plane"""
    return VM.view_planes(source(alpha, px4), full, None, filter)


def view_planes(alpha, px4, full, window=None, filter="bilinear"):
    """R: (4, window h, window w) uint8 of the view, not mirrored"""
    x, y, w, h = (0, 0, full[0], full[1]) if window is None else window
    return result(alpha, resized(alpha, px4, full, filter)[:, y:y + h, x:x + w])


def view_elements(r4, c, dtype, mirror, m, consts, post, warp, tone, enhance):
    """R (view_planes) -> the (oh, ow, c) element bits of a destination of c channels: every later stage sees R as it sees the
    resize's bytes, so this is enhance_model.view_elements"""
    return EM.view_elements(r4, c, dtype, mirror, m, consts, post, warp, tone, enhance)


def conditions(px4, full, filter):
    """what a premultiplied resize of px4 exercises: samples of R' where U's clip is live (0 < R'_3 < 255 and 255 * R'_c // R'_3 >
    255), samples with R'_3 == 0 and a non-zero colour, and the source's samples with alpha 0, 255 and in between"""
    r = resized({"op": "premultiplied"}, px4, full, filter).astype(np.int64)
    a = r[3]
    mid = (a > 0) & (a < 255)
    clip = sum(int(np.count_nonzero(mid & (255 * r[c] // np.where(a == 0, 1, a) > 255))) for c in range(3))
    zero = int(np.count_nonzero((a == 0) & ((r[0] | r[1] | r[2]) != 0)))
    pa = np.asarray(px4[3])
    return {"clip": clip, "zero_alpha_colour": zero, "alpha_0": int(np.count_nonzero(pa == 0)), "alpha_255": int(np.count_nonzero(pa == 255)),
            "alpha_between": int(np.count_nonzero((pa > 0) & (pa < 255)))}


def pattern(w, h, seed=0):
    """the test image (h, w, 4) uint8, R, G, B, A: noise colour; alpha in columns of 0 / 255 / 1 / 254 / noise, and rows of 0 and of
    255 every 7th row; bright colour (>= 200) where alpha is 255 -- next to transparent samples a bicubic resize of the premultiplied
    planes overshoots in the colour past the alpha (U's clip) and undershoots the alpha to 0 under a colour that is not"""
    rng = np.random.default_rng(1000 + seed)
    px = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    x = np.arange(w) % 5
    a = px[..., 3]
    a[:, x == 0], a[:, x == 1], a[:, x == 2], a[:, x == 3] = 0, 255, 1, 254
    a[0::7, :] = 0
    a[3::7, :] = 255
    bright = a == 255
    px[..., :3][bright] = 200 + px[..., :3][bright] % 56
    return px
