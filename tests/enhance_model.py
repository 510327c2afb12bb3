"""An exact restatement of the enhance rule of fpng_amd_decode_batch(_device)_planar_views_enhance / _hwc_views_enhance
(include/fpng_amd.h) that does not use the library -- numpy integers for the degenerate images, numpy
float32 (one rounded operation per call) for the blend:

    W': what the tone stage hands on (W itself without a tone op); planes 0, 1, 2 only
    blend(d, v, f as fp32): t = f32(d) + f32(f * f32(v - d)); 0 <= f <= 1: trunc(t); else 0 if t <= 0, 255 if t >= 255, trunc(t) between
    brightness: d = 0;  color: d = L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16 for the three channels
    sharpness: d = smooth(plane): w < 3 or h < 3, or a sample of the outer frame: the sample itself; else (2 S + 13) // 26 with S the
        sum of the 3 x 3 neighbourhood + 4 x the centre
    E_c = blend(d_c, W'_c, f)

An enhance record here is a dict with ONE of the keys "brightness", "color", "sharpness": factor; {} is a view without an op."""
import numpy as np

import color_model as CM
import post_model as PM
import tone_model as TM
import warp_model as WM


def smooth(plane):
    """Pillow's ImageFilter.SMOOTH of one (h, w) uint8 plane"""
    p = np.asarray(plane, dtype=np.uint8)
    h, w = p.shape
    out = p.copy()
    if h < 3 or w < 3:
        return out
    q = p.astype(np.int64)
    s = 4 * q[1:-1, 1:-1]
    for dy in range(3):
        for dx in range(3):
            s = s + q[dy:h - 2 + dy, dx:w - 2 + dx]
    out[1:-1, 1:-1] = ((2 * s + 13) // 26).astype(np.uint8)
    return out


def blend(d, v, f):
    """Pillow's ImagingBlend(d, v, f) of two uint8 arrays (or numbers), as an x86-64 build computes it"""
    f = np.float32(f)
    d, v = np.asarray(d).astype(np.int64), np.asarray(v).astype(np.int64)
    with np.errstate(over="ignore"):
        p = f * (v - d).astype(np.float32)  # (each numpy call: one fp32 operation, rounded)
        t = d.astype(np.float32) + p
    assert p.dtype == np.float32 and t.dtype == np.float32
    if 0.0 <= float(f) <= 1.0:
        return np.trunc(t).astype(np.int64).astype(np.uint8)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, np.trunc(np.clip(t, 0, 255)))).astype(np.int64).astype(np.uint8)


def apply(enhance, planes):
    """E of the three (h, w) uint8 planes W' (a (3, h, w) array or a list)"""
    planes = [np.ascontiguousarray(p, dtype=np.uint8) for p in planes[:3]]
    if not enhance:
        return np.stack(planes)
    (name, f), = enhance.items()
    if name == "brightness":
        d = [np.zeros_like(p) for p in planes]
    elif name == "color":
        d = [TM.luma(planes)] * 3
    else:
        assert name == "sharpness", name
        d = [smooth(p) for p in planes]
    return np.stack([blend(d[c], planes[c], f) for c in range(3)])


def view_elements(r4, c, dtype, mirror, m, consts, post, warp, tone, enhance):
    """tone_model.view_elements with an enhance record behind the tone record and in front of the blur: (4, oh, ow) bytes of a view,
    not mirrored -> the (oh, ow, c) element bits of a destination of c channels"""
    if not enhance:
        return TM.view_elements(r4, c, dtype, mirror, m, consts, post, warp, tone)
    m = PM.IDENTITY if m is None else m
    px = np.ascontiguousarray(r4.transpose(1, 2, 0))
    b = CM.element_bits_np(CM.apply_np(m, px[..., :3]), "uint8")  # step 1
    planes = [b[..., k] for k in range(3)] + ([px[..., 3]] if c == 4 else [])
    moves = bool(warp) and tuple(float(v) for v in warp["a"]) != WM.IDENTITY
    if moves:  # (the gather mirrors; there is no second mirror)
        planes = [WM.apply_plane(warp, p, mirror, warp["fill"][k]) for k, p in enumerate(planes)]
    e = apply(enhance, TM.apply(tone, planes[:3]))
    z = [PM.apply_plane(post, e[k]) for k in range(3)] + planes[3:]
    if mirror and not moves:
        z = [p[:, ::-1] for p in z]
    scale, bias = (consts[0], consts[1]) if dtype != "uint8" else ([1.0] * 4, [0.0] * 4)
    return np.stack([CM.element_bits_np(p.astype(np.float32), dtype, scale[k], bias[k]) for k, p in enumerate(z)], axis=-1)
