"""An exact restatement of the warp rule of fpng_amd_decode_batch(_device)_planar_views_warp / _hwc_views_warp (include/fpng_amd.h,
INTEGRATION.md section 7) that does not use the library -- Python integers for the fixed-point coefficients, numpy int64 for the
nearest positions and numpy float64 for the bilinear ones (one IEEE double operation per numpy call, in the stated order: nothing is
fused):

    M[q][i] = B[q][mirror ? w - 1 - i : i],  W = warp(M);  the post rule's steps 2 to 4 then run on W, and there is no second mirror
    nearest:  FIX(v) = floor(v * 65536.0 + 0.5);  A0, A1, A3, A4 = FIX(a0), FIX(a1), FIX(a3), FIX(a4);
              A2 = FIX(a2 + a0 * 0.5 + a1 * 0.5), A5 = FIX(a5 + a3 * 0.5 + a4 * 0.5);
              sx = (A2 + x A0 + y A1) >> 16, sy = (A5 + x A3 + y A4) >> 16;  W[y][x] = inside ? M[sy][sx] : fill
    bilinear: xs = (a0 (x + .5) + a1 (y + .5)) + a2, ys likewise;  fill if xs < 0 || xs >= w || ys < 0 || ys >= h;  xs -= .5, ys -= .5;
              xi = floor(xs), yi = floor(ys), dx = xs - xi, dy = ys - yi;  x0 = clamp(xi), x1 = clamp(xi + 1), row clamp(yi);
              v1 = p[x0] + (p[x1] - p[x0]) dx;  v2 the same on row yi + 1 if it is inside, else v1;  W = trunc(v1 + (v2 - v1) dy)

A warp record here is a dict {"a": the six coefficients, "filter": "nearest" | "bilinear", "fill": four bytes, one per file channel};
{} is a view without a warp.  A record whose coefficients are exactly the identity's leaves its view to the post rule, as {} does."""
import math

import numpy as np

import color_model as CM
import post_model as PM

IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def fix(v):
    return int(math.floor(v * 65536.0 + 0.5))


def fixed_coefficients(a):
    a = [float(v) for v in a]
    return [fix(a[0]), fix(a[1]), fix(a[2] + a[0] * 0.5 + a[1] * 0.5), fix(a[3]), fix(a[4]), fix(a[5] + a[3] * 0.5 + a[4] * 0.5)]


def corners_ok(a, w, h):
    """Pillow's check_fixed at the four output corners"""
    return all(abs(x * a[0] + y * a[1] + a[2]) < 32768.0 and abs(x * a[3] + y * a[4] + a[5]) < 32768.0 for x in (0.0, float(w)) for y in (0.0, float(h)))


def warp_plane(a, filter, fill, m):
    """W for the (h, w) uint8 plane m, which is M: already mirrored"""
    m = np.ascontiguousarray(m, dtype=np.uint8)
    h, w = m.shape
    out = np.full((h, w), fill, dtype=np.uint8)
    if filter == "nearest":
        A = fixed_coefficients(a)
        assert all(abs(v) < 2 ** 40 for v in A)  # (int64 holds every sum below)
        x, y = np.arange(w, dtype=np.int64)[None, :], np.arange(h, dtype=np.int64)[:, None]
        sx, sy = (A[2] + x * A[0] + y * A[1]) >> 16, (A[5] + x * A[3] + y * A[4]) >> 16
        inside = (sx >= 0) & (sx < w) & (sy >= 0) & (sy < h)
        out[inside] = m[sy[inside], sx[inside]]
        return out
    assert filter == "bilinear"
    a = [np.float64(v) for v in a]
    xc, yc = (np.arange(w, dtype=np.float64) + 0.5)[None, :], (np.arange(h, dtype=np.float64) + 0.5)[:, None]
    xs, ys = (a[0] * xc + a[1] * yc) + a[2], (a[3] * xc + a[4] * yc) + a[5]
    inside = ~((xs < 0.0) | (xs >= float(w)) | (ys < 0.0) | (ys >= float(h)))
    xs, ys = xs - 0.5, ys - 0.5
    fx, fy = np.floor(xs), np.floor(ys)
    dx, dy = xs - fx, ys - fy
    xi, yi = np.where(inside, fx, 0.0).astype(np.int64), np.where(inside, fy, 0.0).astype(np.int64)
    x0, x1, y0 = np.clip(xi, 0, w - 1), np.clip(xi + 1, 0, w - 1), np.clip(yi, 0, h - 1)
    below = (yi + 1 >= 0) & (yi + 1 < h)
    y1 = np.where(below, yi + 1, y0)  # (the same samples and dx: v2 = v1)
    p = m.astype(np.int64)
    p00, p01, p10, p11 = p[y0, x0], p[y0, x1], p[y1, x0], p[y1, x1]
    v1 = p00.astype(np.float64) + (p01 - p00).astype(np.float64) * dx
    v2 = p10.astype(np.float64) + (p11 - p10).astype(np.float64) * dx
    v = v1 + (v2 - v1) * dy
    out[inside] = np.trunc(v[inside]).astype(np.uint8)
    return out


def apply_plane(warp, plane, mirror=False, fill=None):
    """step 1a for one (h, w) uint8 plane of B (un-mirrored); fill None: the record's fill[0]"""
    m = np.ascontiguousarray(plane, dtype=np.uint8)
    if mirror:
        m = m[:, ::-1]
    if not warp:
        return np.ascontiguousarray(m)
    return warp_plane(warp["a"], warp["filter"], warp["fill"][0] if fill is None else fill, m)


def view_elements(r4, c, dtype, mirror, m, consts, post, warp):
    """post_model.view_elements with a warp record between the colour step's bytes and the blur: (4, oh, ow) bytes of a view, not
    mirrored -> the (oh, ow, c) element bits of a destination of c channels"""
    if not warp or tuple(float(v) for v in warp["a"]) == IDENTITY:  # (the identity is a record without flags: W = M)
        return PM.view_elements(r4, c, dtype, mirror, m, consts, post)
    m = PM.IDENTITY if m is None else m
    px = np.ascontiguousarray(r4.transpose(1, 2, 0))
    b = CM.element_bits_np(CM.apply_np(m, px[..., :3]), "uint8")  # step 1
    planes = [b[..., k] for k in range(3)] + ([px[..., 3]] if c == 4 else [])
    wp = [apply_plane(warp, p, mirror, warp["fill"][k]) for k, p in enumerate(planes)]  # ALL planes; the mirror is in front
    z = [PM.apply_plane(post, p) for p in wp[:3]] + wp[3:]
    scale, bias = (consts[0], consts[1]) if dtype != "uint8" else ([1.0] * 4, [0.0] * 4)
    return np.stack([CM.element_bits_np(p.astype(np.float32), dtype, scale[k], bias[k]) for k, p in enumerate(z)], axis=-1)
