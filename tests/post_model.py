"""An exact restatement of the post rule of fpng_amd_decode_batch(_device)_planar_views_post / _hwc_views_post (include/fpng_amd.h,
INTEGRATION.md section 7) that does not use the library -- numpy integers and math.exp (not np.exp: its vector path need not be
libm's):

    1. B = (uint8_t)rintf(u_c), the colour rule's bytes of the un-mirrored window (color_model.py)
    2. blur, radius R:  p[d] = exp(-0.5 * (d / sigma) * (d / sigma)), ww = p[0] + 2 p[1] + ... in this order,
       k[d] = (int)(0.5 + p[d] / ww * 2^22); tap t = -R .. R has weight k[|t|]; refl(j, n) = j < 0 ? -j : j >= n ? 2 (n - 1) - j : j;
       H[q][i] = pass(sum_t B[q][refl(i + t, w)] k[|t|]), G[q][i] = pass(sum_t H[refl(q + t, h)][i] k[|t|]),
       pass(s) = clamp((2^21 + s) >> 22, 0, 255)
    3. solarize:  S = G >= threshold ? 255 - G : G
    4. posterize: Z = S & (0xFF00 >> bits) & 0xFF
    5. the element: Z, or round_to_dtype(fmaf((float)Z, scale[c], bias[c])); element (q, i) from Z[q][i], mirrored: Z[q][w - 1 - i]

A post record here is a dict with any of the keys "blur": (R, sigma), "solarize": threshold, "posterize": bits; {} is a view
without flags."""
import math

import numpy as np

import color_model as CM

IDENTITY = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], dtype=np.float32)


def blur_weights(radius, sigma):
    """k[0 .. radius] as Python integers"""
    p = [math.exp(-0.5 * (d / sigma) * (d / sigma)) for d in range(radius + 1)]
    ww = p[0]
    for d in range(1, radius + 1):
        ww = ww + 2.0 * p[d]
    return [int(0.5 + p[d] / ww * 4194304.0) for d in range(radius + 1)]


def refl(j, n):
    return -j if j < 0 else 2 * (n - 1) - j if j >= n else j


def _pass(a, k, axis):
    """one pass along `axis` of the (h, w) uint8 array a -> uint8"""
    radius, n = len(k) - 1, a.shape[axis]
    assert radius < n  # (one reflection is enough)
    idx = np.array([refl(j, n) for j in range(-radius, n + radius)], dtype=np.int64)
    wide = np.take(a.astype(np.int64), idx, axis=axis)
    total = np.full(a.shape, 1 << 21, dtype=np.int64)
    for t in range(-radius, radius + 1):
        total += np.take(wide, np.arange(n) + t + radius, axis=axis) * k[abs(t)]
    assert total.max() < 2 ** 31
    return np.clip(total >> 22, 0, 255).astype(np.uint8)


def apply_plane(post, plane):
    """steps 2 to 4 for one (h, w) uint8 plane"""
    g = np.ascontiguousarray(plane, dtype=np.uint8)
    if "blur" in post:
        k = blur_weights(*post["blur"])
        g = _pass(_pass(g, k, 1), k, 0)
    if "solarize" in post:
        g = np.where(g >= post["solarize"], 255 - g.astype(np.int32), g).astype(np.uint8)
    if "posterize" in post:
        g = g & np.uint8((0xFF00 >> post["posterize"]) & 0xFF)
    return g


def view_elements(r4, c, dtype, mirror, m, consts, post):
    """color_model.view_elements with a post record behind the matrix (m None: the identity): (4, oh, ow) bytes of a view, not
    mirrored -> the (oh, ow, c) element bits of a destination of c channels"""
    m = IDENTITY if m is None else m
    if not post:
        return CM.view_elements(r4, c, dtype, mirror, m, consts)
    px = np.ascontiguousarray(r4.transpose(1, 2, 0))
    b = CM.element_bits_np(CM.apply_np(m, px[..., :3]), "uint8")  # step 1
    z = [apply_plane(post, b[..., k]) for k in range(3)]
    if c == 4:
        z.append(px[..., 3])
    if mirror:
        z = [p[:, ::-1] for p in z]
    scale, bias = (consts[0], consts[1]) if dtype != "uint8" else ([1.0] * 4, [0.0] * 4)
    return np.stack([CM.element_bits_np(p.astype(np.float32), dtype, scale[k], bias[k]) for k, p in enumerate(z)], axis=-1)
