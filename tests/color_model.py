"""An exact restatement of the colour rule of fpng_amd_decode_batch(_device)_planar_views_color / _hwc_views_color
(include/fpng_amd.h) that does not use the library:

    t_c = fmaf(m[c][2], b, fmaf(m[c][1], g, fmaf(m[c][0], r, m[c][3])))          IEEE binary32, one rounding per fmaf
    u_c = fminf(fmaxf(t_c, 0.0f), 255.0f)                                         (-0.0f -> +0.0f)
    uint8:  rint(u_c), ties to even          float:  round_to_dtype(fmaf(u_c, scale[c], bias[c])), fp32 first, then the narrow type

Two texts of it:

  * the SCALAR one in integers (fma32, apply, element_bits): every binary32 value is n / 2^k with Python integers, a * b + c is
    formed exactly and rounded ONCE to 24 bits (or to the quantum 2^-149 of the subnormals), ties to even.  This is the reference.
  * the ARRAY one (fma32_np, apply_np, element_bits_np) for whole views: a * b is exact in float64 (24 + 24 bits), TwoSum gives
    the exact error of its float64 sum with c, and the sum is nudged to ROUND-TO-ODD (an inexact sum with an even last bit moves
    one step towards the error), after which the conversion to binary32 rounds correctly -- 53 >= 24 + 2 bits (Boldo and
    Melquiond).  It is NOT "float64, then round", which errs where the float64 sum lands on a binary32 tie;
    tests/test_views_color_cpu.py holds it against the scalar text on ties, clamps and random values.

Values are finite and far from binary32's overflow (the library refuses entries beyond 65536)."""
import math

import numpy as np


def _ratio(x):
    """a finite float -> (n, k) with x == n / 2^k"""
    n, d = float(x).as_integer_ratio()
    return n, d.bit_length() - 1


def _round(n, k, prec, qmin):
    """n / 2^k rounded to `prec` significant bits, ties to even, with the quantum never below 2^qmin -> a Python float (exact)"""
    if n == 0:
        return 0.0
    sign, n = (-1.0, -n) if n < 0 else (1.0, n)
    shift = max(n.bit_length() - prec, k + qmin)  # bits of n below the result's last place
    if shift > 0:
        q, rem, half = n >> shift, n & ((1 << shift) - 1), 1 << (shift - 1)
        if rem > half or (rem == half and (q & 1)):
            q += 1
        return sign * math.ldexp(q, shift - k)
    return sign * math.ldexp(n, -k)


def fma32(a, b, c):
    """fmaf(a, b, c) for binary32 values held in Python floats: exact product and sum, ONE rounding"""
    (na, ka), (nb, kb), (nc, kc) = _ratio(a), _ratio(b), _ratio(c)
    n, k = na * nb, ka + kb
    top = max(k, kc)
    return _round((n << (top - k)) + (nc << (top - kc)), top, 24, -149)


def f32(x):
    """a Python float (an exact binary64 value) -> the nearest binary32 value"""
    return _round(*_ratio(x), 24, -149)


def apply(m, rgb):
    """u_c of the rule, c = 0, 1, 2.  m: (3, 4) binary32 values; rgb: three bytes"""
    r, g, b = (float(int(v)) for v in rgb)
    out = []
    for c in range(3):
        t = fma32(float(m[c][2]), b, fma32(float(m[c][1]), g, fma32(float(m[c][0]), r, float(m[c][3]))))
        out.append(min(max(t, 0.0), 255.0) + 0.0)  # (max(-0.0, 0.0) may be either zero in Python too: + 0.0 makes it +0.0)
    return out


_NARROW = {"float16": (11, -24, 16), "bfloat16": (8, -133, 128)}  # significant bits, the smallest subnormal's exponent, 2^this overflows


def element_bits(u, dtype, scale=1.0, bias=0.0):
    """the element a destination of `dtype` holds for u_c (or for the alpha byte as a float), as its bits"""
    if dtype == "uint8":
        return int(round(u))  # (Python rounds ties to even)
    f = fma32(float(u), float(scale), float(bias))
    if dtype == "float32":
        return int(np.float32(f).view(np.uint32))
    prec, qmin, emax = _NARROW[dtype]
    h = _round(*_ratio(f), prec, qmin)
    if abs(h) >= math.ldexp(1.0, emax):
        h = math.copysign(math.inf, h)
    if dtype == "float16":
        return int(np.float16(h).view(np.uint16))  # (exact: h is a binary16 value)
    return int(np.float32(h).view(np.uint32)) >> 16  # (exact: h is a bfloat16 value, the top half of its binary32 form)


# ---- the same for arrays ----
def fma32_np(a, b, c):
    """fmaf(a, b, c) elementwise for float32 arrays (broadcast) -> float32, each element rounded once"""
    a, b, c = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (a, b, c))
    p = a * b  # exact: 48 bits
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)  # TwoSum: p + c == s + err exactly
    even = (s.view(np.int64) & 1) == 0
    odd = np.nextafter(s, np.where(err > 0, np.inf, -np.inf))
    s = np.where((err != 0) & even, odd, s)  # round to odd
    return s.astype(np.float32)


def apply_np(m, rgb):
    """u of the rule for rgb (..., 3) uint8 under m (3, 4) -> (..., 3) float32"""
    m = np.asarray(m, dtype=np.float32)
    px = np.asarray(rgb, dtype=np.uint8).astype(np.float32)
    r, g, b = px[..., 0], px[..., 1], px[..., 2]
    out = np.empty(px.shape, dtype=np.float32)
    for c in range(3):
        t = fma32_np(m[c, 2], b, fma32_np(m[c, 1], g, fma32_np(m[c, 0], r, m[c, 3])))
        out[..., c] = np.minimum(np.maximum(t, np.float32(0.0)), np.float32(255.0)) + np.float32(0.0)
    return out


def element_bits_np(u, dtype, scale=1.0, bias=0.0):
    """element_bits for a float32 array -> uint8 / uint32 / uint16 bits"""
    u = np.asarray(u, dtype=np.float32)
    if dtype == "uint8":
        return np.rint(u).astype(np.uint8)  # (ties to even)
    f = fma32_np(u, np.float32(scale), np.float32(bias))
    if dtype == "float32":
        return f.view(np.uint32)
    if dtype == "float16":
        return f.astype(np.float16).view(np.uint16)  # (numpy's conversion rounds to nearest even, subnormals included)
    w = f.view(np.uint32)
    return ((w + np.uint32(0x7FFF) + ((w >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)  # (finite values)


def view_elements(r4, c, dtype, mirror, m, consts):
    """(4, oh, ow) bytes of a view -- what the plain views call's resize gives, not mirrored -> the (oh, ow, c) element bits that a
    destination of c channels holds under matrix m and consts = (scale[4], bias[4]): file channels 0 .. 2 through the matrix, a
    fourth one past it"""
    px = r4[:, :, ::-1] if mirror else r4
    px = np.ascontiguousarray(px.transpose(1, 2, 0))
    u = apply_np(m, px[..., :3])
    scale, bias = (consts[0], consts[1]) if dtype != "uint8" else ([1.0] * 4, [0.0] * 4)
    chans = [element_bits_np(u[..., k], dtype, scale[k], bias[k]) for k in range(3)]
    if c == 4:
        chans.append(element_bits_np(px[..., 3].astype(np.float32), dtype, scale[3], bias[3]))
    return np.stack(chans, axis=-1)
