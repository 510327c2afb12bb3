"""An exact restatement of the tone rule of fpng_amd_decode_batch(_device)_planar_views_tone / _hwc_views_tone (include/fpng_amd.h,
INTEGRATION.md section 7) that does not use the library -- numpy and Python integers for the counts, Python floats (IEEE doubles, one
operation per expression) for autocontrast, numpy float32 (one rounded operation per call) for contrast:

    W: the view's un-mirrored uint8 window as the post stage loads it (B of the post rule, or the warp's W); planes 0, 1, 2 only
    h_c[v]: the count of byte v in plane c;  h_L[v]: the count of L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16
    autocontrast, per channel: lo, hi the first and last non-zero bin; hi <= lo: identity; scale = 255.0 / (hi - lo),
        offset = -lo * scale, lut[v] = clamp(int(v * scale + offset), 0, 255)
    equalize, per channel: fewer than two non-zero bins: identity; step = (sum h - h[last non-zero]) // 255; 0: identity;
        n = step // 2; for v: lut[v] = min(255, n // step); n += h[v]
    contrast(factor as fp32): mean = (2 sum v h_L[v] + N) // (2 N); t = f32(mean) + f32(factor * f32(v - mean));
        0 <= factor <= 1: lut[v] = trunc(t); else 0 if t <= 0, 255 if t >= 255, trunc(t) between; one table for the three channels
    W'_c = lut_c[W_c]

A tone record here is a dict with ONE of the keys "autocontrast": True, "equalize": True, "contrast": factor; {} is a view without an
op."""
import numpy as np

import color_model as CM
import post_model as PM
import warp_model as WM


def luma(planes):
    r, g, b = (np.asarray(planes[k]).astype(np.int64) for k in range(3))
    return ((19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16).astype(np.uint8)


def histograms(planes):
    """(4, 256) Python-sized counts (int64) of the three (h, w) uint8 planes and of their L"""
    return np.stack([np.bincount(np.asarray(p, dtype=np.uint8).ravel(), minlength=256).astype(np.int64) for p in (planes[0], planes[1], planes[2], luma(planes))])


def autocontrast_lut(h):
    h = [int(x) for x in h]
    nz = [v for v in range(256) if h[v]]
    if not nz or nz[-1] <= nz[0]:
        return np.arange(256, dtype=np.uint8)
    lo, hi = nz[0], nz[-1]
    scale = 255.0 / (hi - lo)
    offset = -lo * scale
    return np.array([min(max(int(v * scale + offset), 0), 255) for v in range(256)], dtype=np.uint8)


def equalize_entries(h):
    """the UNCLAMPED entries of equalize (Python integers), or None for the identity"""
    h = [int(x) for x in h]
    nz = [x for x in h if x]
    if len(nz) < 2:
        return None
    step = (sum(nz) - nz[-1]) // 255
    if not step:
        return None
    out, n = [], step // 2
    for v in range(256):
        out.append(n // step)
        n += h[v]
    return out


def equalize_lut(h):
    e = equalize_entries(h)
    return np.arange(256, dtype=np.uint8) if e is None else np.array([min(255, x) for x in e], dtype=np.uint8)


def contrast_mean(h_l):
    h_l = [int(x) for x in h_l]
    n = sum(h_l)
    return (2 * sum(v * x for v, x in enumerate(h_l)) + n) // (2 * n)


def contrast_lut_of_mean(mean, factor):
    f = np.float32(factor)
    d = (np.arange(256, dtype=np.int64) - int(mean)).astype(np.float32)
    with np.errstate(over="ignore"):
        t = np.float32(mean) + f * d  # (each numpy call: one fp32 operation, rounded)
    assert t.dtype == np.float32
    if 0.0 <= float(f) <= 1.0:
        return np.trunc(t).astype(np.int64).astype(np.uint8)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, np.trunc(np.clip(t, 0, 255)))).astype(np.int64).astype(np.uint8)


def contrast_lut(h_l, factor):
    return contrast_lut_of_mean(contrast_mean(h_l), factor)


def luts(tone, hist):
    """the (3, 256) uint8 tables of a tone record from the (4, 256) histograms"""
    if tone.get("autocontrast"):
        return np.stack([autocontrast_lut(hist[c]) for c in range(3)])
    if tone.get("equalize"):
        return np.stack([equalize_lut(hist[c]) for c in range(3)])
    if "contrast" in tone:
        return np.stack([contrast_lut(hist[3], tone["contrast"])] * 3)
    return np.stack([np.arange(256, dtype=np.uint8)] * 3)


def apply(tone, planes):
    """W' of the three (h, w) uint8 planes W (a (3, h, w) array or a list)"""
    planes = [np.ascontiguousarray(p, dtype=np.uint8) for p in planes[:3]]
    if not tone:
        return np.stack(planes)
    t = luts(tone, histograms(planes))
    return np.stack([t[c][planes[c]] for c in range(3)])


def view_elements(r4, c, dtype, mirror, m, consts, post, warp, tone):
    """warp_model.view_elements with a tone record behind the warp and in front of the blur: (4, oh, ow) bytes of a view, not
    mirrored -> the (oh, ow, c) element bits of a destination of c channels"""
    if not tone:
        return WM.view_elements(r4, c, dtype, mirror, m, consts, post, warp)
    m = PM.IDENTITY if m is None else m
    px = np.ascontiguousarray(r4.transpose(1, 2, 0))
    b = CM.element_bits_np(CM.apply_np(m, px[..., :3]), "uint8")  # step 1
    planes = [b[..., k] for k in range(3)] + ([px[..., 3]] if c == 4 else [])
    moves = bool(warp) and tuple(float(v) for v in warp["a"]) != WM.IDENTITY
    if moves:  # (the gather mirrors; there is no second mirror)
        planes = [WM.apply_plane(warp, p, mirror, warp["fill"][k]) for k, p in enumerate(planes)]
    toned = apply(tone, planes[:3])
    z = [PM.apply_plane(post, toned[k]) for k in range(3)] + planes[3:]
    if mirror and not moves:
        z = [p[:, ::-1] for p in z]
    scale, bias = (consts[0], consts[1]) if dtype != "uint8" else ([1.0] * 4, [0.0] * 4)
    return np.stack([CM.element_bits_np(p.astype(np.float32), dtype, scale[k], bias[k]) for k, p in enumerate(z)], axis=-1)
