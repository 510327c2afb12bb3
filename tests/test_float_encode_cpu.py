"""No-GPU tests of the float encode interface (fpng_amd_encode_submit_planar_float): the exported entry points, denormalize_constants,
source_layout_float on CPU tensor views of the three dtypes, the descriptor make_batch_float builds, and the quantiser itself --
fpng_amd_quantize_float runs on the host the text the kernels compile (csrc/quantize.h) -- against the rule

    y = fmaf((float)x, scale, bias);  byte = y is NaN ? 0 : min(max(rint(y), 0), 255)        (ties to even)

The ORACLE quantiser below is numpy only and never calls the library: y in float64 (the product is exact there), then the rule.
Float64-then-round can differ from one fp32 fma only within an fp32 ulp of a tie, so the image generators (float_image, used by the
GPU tests too) resample elements whose y lies within 2^-10 of k + 0.5 -- at most 1 % of an image, asserted -- and the ties
themselves are tested with values where both are exact.  (Where the fma cannot round at all -- 16-bit elements, a scale of few bits,
no bias -- the oracle is exact everywhere and float_image leaves the image as drawn, ties and all: see there.)"""
import ctypes as C

import numpy as np
import pytest
import torch

import fpng_amd
from fpng_amd import _lib
from fpng_amd.api import Encoder, denormalize_constants, normalize_constants, source_layout_float, source_layout_planar

DTYPES = [(torch.float32, 4, 0), (torch.float16, 2, 1), (torch.bfloat16, 2, 2)]
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


# ---- element types as numpy sees them: code 0 = float32, 1 = float16, 2 = bfloat16 held as its uint16 bits ----
def to_elements(values, code):
    """float64 values -> the stored elements (np.float32 / np.float16 / np.uint16 holding bf16 bits), rounded to nearest even"""
    v = np.asarray(values, dtype=np.float64)
    if code == 0:
        return v.astype(np.float32)
    if code == 1:
        with np.errstate(over="ignore"):
            return v.astype(np.float16)
    t = torch.from_numpy(np.ascontiguousarray(v.astype(np.float32))).to(torch.bfloat16)
    return t.view(torch.int16).numpy().view(np.uint16).reshape(v.shape)


def element_values(elems, code):
    """the stored elements -> their exact values as float64"""
    with np.errstate(invalid="ignore"):  # (signalling NaNs)
        if code == 2:
            return (elems.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
        return elems.astype(np.float64)


def oracle_quantize(x, scale, bias):
    """x: float64 values of the source elements; scale, bias: float32 constants -> bytes, by the rule, in float64"""
    with np.errstate(invalid="ignore", over="ignore"):
        y = np.asarray(x, dtype=np.float64) * np.float64(np.float32(scale)) + np.float64(np.float32(bias))
        r = np.clip(np.rint(y), 0.0, 255.0)  # (np.rint: ties to even)
    return np.where(np.isnan(y), 0.0, r).astype(np.uint8)


def near_tie(y):
    with np.errstate(invalid="ignore"):
        return (y >= -1.0) & (y <= 256.0) & (np.abs(y - np.floor(y) - 0.5) < 2.0 ** -10)


def _significant_bits(v):
    """bits from the first to the last set bit of a float32's significand"""
    m = (int(np.float32(v).view(np.uint32)) & 0x7FFFFF) | 0x800000
    return 24 - (m & -m).bit_length() + 1


def float_image(img, code, scale, bias, rng, to_float=None):
    """img (h, w, c) uint8 -> (elements (h, w, c) of type `code`, the bytes (h, w, c) the oracle gives for them).  An element is
    to_float((byte + d) / 255, channel) with |d| < 0.45 (to_float: identity if None); elements that quantise within 2^-10 of a tie
    are drawn again (new d, then a new byte too): at most 1 % of the image, asserted."""
    h, w, c = img.shape
    to_float = to_float or (lambda u, ch: u)
    sc, bi = np.asarray(scale, dtype=np.float32), np.asarray(bias, dtype=np.float32)

    def make(b):
        u = (b.astype(np.float64) + rng.uniform(-0.45, 0.45, b.shape)) / 255.0
        return to_elements(np.stack([to_float(u[..., ch], ch) for ch in range(c)], axis=-1), code)

    def y_of(e):
        return element_values(e, code) * sc[:c].astype(np.float64) + bi[:c].astype(np.float64)
    el = make(img)
    touched = np.zeros(img.shape, dtype=bool)
    b = img.copy()
    # Where the fma cannot round there is nothing to keep away from: a 16-bit element has 11 (f16) or 8 (bf16) significant bits, and
    # with a zero bias and a scale of at most 24 - that many bits (255: eight) its product is exact in fp32 as it is in float64, ties
    # included.  Those images are left as drawn -- bf16's coarse steps put whole runs of a 128 byte ON 127.5, far more than 1 %.
    exact = code != 0 and not bi[:c].any() and all(_significant_bits(v) + (11 if code == 1 else 8) <= 24 for v in sc[:c])
    for attempt in range(0 if exact else 64):
        bad = near_tie(y_of(el))
        if not bad.any():
            break
        touched |= bad
        if attempt >= 4:
            b = np.where(bad, rng.integers(0, 256, b.shape, dtype=np.uint8), b)
        el = np.where(bad, make(b), el)
    else:
        assert exact, "float_image: elements stay near a tie"
    assert touched.sum() <= max(1, img.size // 100), f"float_image resampled {touched.sum()} of {img.size} elements (more than 1 %)"
    x = element_values(el, code)
    return el, np.stack([oracle_quantize(x[..., ch], sc[ch], bi[ch]) for ch in range(c)], axis=-1)


def lib_quantize(elems, code, scale, bias):
    lib = _lib.load()
    src = np.ascontiguousarray(elems)
    dst = np.empty(src.size, dtype=np.uint8)
    assert lib.fpng_amd_quantize_float(src.ctypes.data, code, float(np.float32(scale)), float(np.float32(bias)), dst.ctypes.data, src.size) == 0
    return dst.reshape(src.shape)


# ---- the interface ----
def test_entry_points_and_record(built_lib):
    lib = _lib.load()
    for name in ("fpng_amd_encode_submit_planar_float", "fpng_amd_quantize_float"):
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None
    assert lib.fpng_amd_abi_version() == 5  # (new entry points, the same ABI version)
    assert C.sizeof(_lib.FloatFormat) == 40 and C.sizeof(_lib.ImagePlanar) == 56
    for name in ("denormalize_constants", "source_layout_float"):
        assert hasattr(fpng_amd, name)
    assert hasattr(Encoder, "make_batch_float") and hasattr(Encoder, "submit_float")


def test_null_arguments_are_refused_without_a_device(built_lib):
    lib = _lib.load()
    fmt = _lib.FloatFormat()
    arr = (_lib.ImagePlanar * 1)()
    t = C.c_uint64(7)
    fn = lib.fpng_amd_encode_submit_planar_float
    assert fn(None, arr, 1, C.byref(fmt), 0, C.byref(t)) == -1
    assert fn(None, None, 1, C.byref(fmt), 0, C.byref(t)) == -1
    assert fn(None, arr, 1, None, 0, C.byref(t)) == -1
    assert t.value == 7
    assert lib.fpng_amd_quantize_float(None, 0, 1.0, 0.0, None, 4) == -1
    assert lib.fpng_amd_quantize_float(None, 0, 1.0, 0.0, None, 0) == 0
    one = np.zeros(1, dtype=np.float32)
    out = np.zeros(1, dtype=np.uint8)
    assert lib.fpng_amd_quantize_float(one.ctypes.data, 3, 1.0, 0.0, out.ctypes.data, 1) == -1


def test_denormalize_constants():
    mean, std = IMAGENET_MEAN, IMAGENET_STD
    scale, bias = denormalize_constants(mean, std)
    assert scale.dtype == bias.dtype == np.float32 and scale.shape == bias.shape == (4,)
    for c in range(3):
        assert scale[c] == np.float32(255.0 * std[c]) and bias[c] == np.float32(255.0 * mean[c])
    assert scale[3] == 255.0 and bias[3] == 0.0  # (missing channels: plain [0, 1])
    scale, bias = denormalize_constants(mean + (0.5,), std + (0.25,))
    assert scale[3] == np.float32(63.75) and bias[3] == np.float32(127.5)
    scale, bias = denormalize_constants([0.5], [0.5], max_value=1.0)
    assert list(scale) == [0.5, 1.0, 1.0, 1.0] and list(bias) == [0.5, 0.0, 0.0, 0.0]
    scale, bias = denormalize_constants([], [])
    assert np.all(scale == 255.0) and np.all(bias == 0)
    for bad in (((0.5, 0.5), (0.5,)), ((0.5,) * 5, (0.5,) * 5), ((0.5,), (0.0,)), ((float("nan"),), (1.0,)), ((0.5,), (float("inf"),))):
        with pytest.raises(ValueError):
            denormalize_constants(*bad)
    with pytest.raises(ValueError):
        denormalize_constants([0.5], [0.5], max_value=0.0)


def test_byte_to_float32_to_byte_is_the_identity(built_lib):
    """normalize_constants, then denormalize_constants through the library's quantiser: all 256 bytes, ImageNet's mean / std"""
    ns, nb = normalize_constants(IMAGENET_MEAN, IMAGENET_STD)
    ds, db = denormalize_constants(IMAGENET_MEAN, IMAGENET_STD)
    bytes_ = np.arange(256, dtype=np.uint8)
    for c in range(4):
        x = (bytes_.astype(np.float64) * np.float64(ns[c]) + np.float64(nb[c])).astype(np.float32)  # (what the float decode stores, to within its last bit)
        assert np.array_equal(lib_quantize(x, 0, ds[c], db[c]), bytes_), f"channel {c}"
        assert np.array_equal(oracle_quantize(x.astype(np.float64), ds[c], db[c]), bytes_)


@pytest.mark.parametrize("dtype,e,code", DTYPES)
def test_source_layout_float(dtype, e, code):
    """the uint8 rules on strides counted in elements; pitches and pointer offsets in bytes"""
    for c, h, w in ((3, 5, 7), (4, 5, 7), (3, 1, 9), (4, 9, 1), (3, 1, 1)):  # contiguous; one row; one column
        t = torch.zeros(c, h, w, dtype=dtype)
        assert source_layout_float(t) == (t.data_ptr(), (w * e if h > 1 else 0), h * w * e, code)
    n = torch.zeros(5, 3, 6, 11, dtype=dtype)
    assert source_layout_float(n[2]) == (n.data_ptr() + 2 * 3 * 66 * e, 11 * e, 66 * e, code)
    assert [source_layout_float(v)[0] for v in list(n)] == [n.data_ptr() + i * 3 * 66 * e for i in range(5)]
    q = torch.zeros(4, 6, 11, dtype=dtype)
    assert source_layout_float(q[:3]) == (q.data_ptr(), 11 * e, 66 * e, code)
    t = torch.zeros(3, 40, 50, dtype=dtype)
    assert source_layout_float(t[:, 7:19, 3:44]) == (t.data_ptr() + (7 * 50 + 3) * e, 50 * e, 2000 * e, code)  # a crop
    assert source_layout_float(t[:, 7:8, 3:44]) == (t.data_ptr() + (7 * 50 + 3) * e, 0, 2000 * e, code)  # ... of one row
    assert source_layout_float(t[:, 7:19, 3:4]) == (t.data_ptr() + (7 * 50 + 3) * e, 50 * e, 2000 * e, code)  # ... of one column
    buf = torch.zeros(4, 10, 64, dtype=dtype)
    assert source_layout_float(buf[:, :, :33]) == (buf.data_ptr(), 64 * e, 640 * e, code)  # padded rows
    t = torch.zeros(3, 6, 11, dtype=dtype)
    assert source_layout_float(t, bottom_up=True) == (t.data_ptr() + 5 * 11 * e, -11 * e, 66 * e, code)
    assert source_layout_float(t, order="bgr") == (t.data_ptr() + 2 * 66 * e, 11 * e, -66 * e, code)
    assert source_layout_float(t, order="BGR", bottom_up=True) == (t.data_ptr() + (2 * 66 + 5 * 11) * e, -11 * e, -66 * e, code)
    assert source_layout_float(q, order="abgr") == (q.data_ptr() + 3 * 66 * e, 11 * e, -66 * e, code)
    assert source_layout_float(q, order="rgba") == source_layout_float(q, order="rgb")
    # the same view as bytes gives the same pointer and pitches
    assert source_layout_float(t[:, 1:5, 2:9], "bgr", True)[:3] == source_layout_planar(t[:, 1:5, 2:9].view(torch.uint8), "bgr", True)


@pytest.mark.parametrize("dtype,e,code", DTYPES)
def test_source_layout_float_refusals(dtype, e, code):
    t = torch.zeros(3, 6, 11, dtype=dtype)
    q = torch.zeros(4, 6, 11, dtype=dtype)
    for bad in ("bgra", "argb", "bgr", "rgbx", "xyz"):
        with pytest.raises(ValueError):
            source_layout_float(q, order=bad)
    for bad in ("rgba", "abgr", "rbg", ""):
        with pytest.raises(ValueError):
            source_layout_float(t, order=bad)
    for other in (torch.uint8, torch.int8, torch.float64, torch.int32):
        with pytest.raises(ValueError):
            source_layout_float(torch.zeros(3, 4, 5, dtype=other))
    for shape in ((2, 3, 4, 5), (4, 5), (2, 4, 5), (5, 4, 5)):  # rank, plane count
        with pytest.raises(ValueError):
            source_layout_float(torch.zeros(*shape, dtype=dtype))
    with pytest.raises(ValueError):
        source_layout_float("not a tensor")
    with pytest.raises(ValueError):  # an interleaved view: stride(2) != 1
        source_layout_float(torch.zeros(6, 11, 3, dtype=dtype).permute(2, 0, 1))
    for view in (t[:, :, ::2], t[:1].expand(3, 6, 11), t[:, :1].expand(3, 6, 11), torch.as_strided(t, (3, 6, 11), (66, 10, 1)),
                 torch.as_strided(t, (3, 6, 11), (65, 11, 1)), torch.as_strided(t, (3, 6, 11), (11, 33, 1))):  # overlapping rows or planes
        with pytest.raises(ValueError):
            source_layout_float(view)
    assert source_layout_float(torch.as_strided(t, (3, 5, 10), (66, 11, 1)))  # (the same with room: fine)


@pytest.mark.parametrize("dtype,e,code", DTYPES)
def test_make_batch_float_on_cpu_tensors(dtype, e, code):
    big = torch.zeros(4, 20, 30, dtype=dtype)
    views = [big, big[:3, 2:12, 5:25], big[:3]]
    outs = [torch.zeros(100, dtype=torch.uint8), torch.zeros(200, dtype=torch.uint8), torch.zeros(300, dtype=torch.uint8)]
    images, outs_, arr, fmt = Encoder.make_batch_float(views, outs, order=["rgba", "rgb", "bgr"], bottom_up=[False, True, False],
                                                       mean=(0.5, 0.25, 0.125), std=(0.5, 0.25, 2.0))
    assert images is views and outs_ is outs and len(arr) == 3
    assert (fmt.dtype, fmt.reserved) == (code, 0)
    sc, bi = denormalize_constants((0.5, 0.25, 0.125), (0.5, 0.25, 2.0))
    assert list(fmt.scale) == [float(v) for v in sc] and list(fmt.bias) == [float(v) for v in bi]
    a = arr[0]
    assert (a.d_pixels, a.row_pitch, a.plane_pitch, a.w, a.h, a.num_chans, a.reserved) == (big.data_ptr(), 30 * e, 600 * e, 30, 20, 4, 0)
    assert (a.d_out, a.out_cap) == (outs[0].data_ptr(), 100)
    a = arr[1]
    assert (a.d_pixels, a.row_pitch, a.plane_pitch, a.w, a.h, a.num_chans) == (big.data_ptr() + (2 * 30 + 5 + 9 * 30) * e, -30 * e, 600 * e, 20, 10, 3)
    a = arr[2]
    assert (a.d_pixels, a.row_pitch, a.plane_pitch, a.w, a.h, a.num_chans, a.out_cap) == (big.data_ptr() + 1200 * e, 30 * e, -600 * e, 30, 20, 3, 300)
    # scale / bias given directly, padded with 255 and 0; neither: plain [0, 1]
    fmt = Encoder.make_batch_float(views[:1], outs[:1], scale=[127.5] * 3, bias=[127.5])[3]
    assert list(fmt.scale) == [127.5, 127.5, 127.5, 255.0] and list(fmt.bias) == [127.5, 0.0, 0.0, 0.0]
    fmt = Encoder.make_batch_float(views[:1], outs[:1])[3]
    assert list(fmt.scale) == [255.0] * 4 and list(fmt.bias) == [0.0] * 4
    nchw = torch.zeros(3, 3, 4, 5, dtype=dtype)
    arr = Encoder.make_batch_float(list(nchw), outs)[2]  # list(nchw_batch) is a valid `images`
    assert [a.d_pixels for a in arr] == [nchw.data_ptr() + i * 60 * e for i in range(3)]
    for kw in (dict(mean=[0.5]), dict(std=[0.5]), dict(mean=[0.5], std=[0.5], scale=[1.0]), dict(scale=[float("inf")]), dict(bias=[float("nan")]),
               dict(scale=[1.0] * 5)):
        with pytest.raises(ValueError):
            Encoder.make_batch_float(views[:1], outs[:1], **kw)


def test_mixed_dtypes_are_refused():
    ims = [torch.zeros(3, 2, 2, dtype=torch.float32), torch.zeros(3, 2, 2, dtype=torch.float16)]
    outs = [torch.zeros(64, dtype=torch.uint8)] * 2
    with pytest.raises(ValueError, match="one dtype"):
        Encoder.make_batch_float(ims, outs)
    with pytest.raises(ValueError):
        Encoder.make_batch_float([torch.zeros(3, 2, 2, dtype=torch.uint8)], outs[:1])
    e = Encoder.__new__(Encoder)  # (no device: an encoder object without a handle)
    e.lib, e.h = _lib.load(), None
    with pytest.raises(ValueError, match="CUDA"):
        Encoder.submit_float(e, ims[:1], outs[:1])


# ---- the quantiser against the rule ----
def _rule(y):
    """the rule on an exact y (a python float holding the exact value)"""
    if y != y:
        return 0
    r = float(np.rint(np.float64(y))) if abs(y) < 1e15 else y
    return int(min(max(r, 0.0), 255.0))


@pytest.mark.parametrize("code", [0, 1, 2])
def test_exact_ties(built_lib, code):
    ks = np.arange(-2, 258, dtype=np.float64)
    x = ks + 0.5
    el = to_elements(x, code)
    exact = element_values(el, code) == x  # the k + 0.5 this dtype holds exactly (bf16: up to 127.5; the others all)
    assert exact.sum() == (130 if code == 2 else 260)
    el, x = el[exact], x[exact]
    for scale, bias in ((1.0, 0.0), (0.5, 0.25)):
        want = np.array([_rule(v * scale + bias) for v in x], dtype=np.uint8)  # (exact in float64 and in one fp32 fma alike)
        assert np.array_equal(lib_quantize(el, code, scale, bias), want), f"scale {scale} bias {bias}"
        assert np.array_equal(oracle_quantize(x, scale, bias), want)
    got = dict(zip(x.tolist(), lib_quantize(el, code, 1.0, 0.0).tolist()))
    assert (got[-1.5], got[-0.5], got[0.5], got[1.5], got[2.5], got[3.5]) == (0, 0, 0, 2, 2, 4)
    if code != 2:
        assert (got[253.5], got[254.5], got[255.5], got[256.5]) == (254, 254, 255, 255)
    else:  # 254.5 = 509 / 2 needs nine bits; 254 and 255 +- the dtype's step around them do not tie
        assert lib_quantize(to_elements([254.0, 255.0, 256.0, 300.0], 2), 2, 1.0, 0.0).tolist() == [254, 255, 255, 255]


@pytest.mark.parametrize("code", [0, 1, 2])
def test_special_values(built_lib, code):
    huge = 6.0e4 if code == 1 else 1.0e30  # (f16's largest values are near 65504)
    x = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, huge, -huge, 1.0, -1.0])
    el = to_elements(x, code)
    assert lib_quantize(el, code, 255.0, 0.0).tolist() == [0, 255, 0, 0, 0, 255, 0, 255, 0]
    assert lib_quantize(el, code, 1.0, 0.0).tolist() == [0, 255, 0, 0, 0, 255, 0, 1, 0]
    assert lib_quantize(el, code, -1.0, 100.0).tolist() == [0, 0, 255, 100, 100, 0, 255, 99, 101]
    assert lib_quantize(el, code, 0.0, 7.0).tolist() == [0, 0, 0, 7, 7, 7, 7, 7, 7]  # inf * 0 is NaN -> 0
    assert oracle_quantize(element_values(el, code), 0.0, 7.0).tolist() == [0, 0, 0, 7, 7, 7, 7, 7, 7]
    # NaNs of every kind: quiet, signalling, either sign
    if code == 0:
        nans = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF], dtype=np.uint32).view(np.float32)
    elif code == 1:
        nans = np.array([0x7E00, 0xFE00, 0x7C01, 0xFC01, 0x7FFF], dtype=np.uint16).view(np.float16)
    else:
        nans = np.array([0x7FC0, 0xFFC0, 0x7F81, 0xFF81, 0x7FFF], dtype=np.uint16)
    assert lib_quantize(nans, code, 255.0, 3.0).tolist() == [0] * 5


@pytest.mark.parametrize("code", [1, 2])
def test_every_16_bit_pattern(built_lib, code):
    bits = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    el = bits.view(np.float16) if code == 1 else bits
    # (scale 255 has eight significant bits, an element at most eleven: the product is exact in fp32 too, and (k + 0.5) / 255 is
    # no binary fraction, so no pattern lies on or near a tie)
    assert np.array_equal(lib_quantize(el, code, 255.0, 0.0), oracle_quantize(element_values(el, code), 255.0, 0.0))


def test_float32_samples_against_the_oracle(built_lib):
    rng = np.random.default_rng(21)
    x = rng.uniform(-0.6, 1.6, 200000).astype(np.float32)
    for scale, bias in ((255.0, 0.0), (58.395, 123.675), (-255.0, 255.0)):
        s32, b32 = np.float32(scale), np.float32(bias)
        y = x.astype(np.float64) * np.float64(s32) + np.float64(b32)
        keep = ~near_tie(y)
        assert keep.mean() > 0.99
        assert np.array_equal(lib_quantize(x[keep], 0, s32, b32), oracle_quantize(x[keep].astype(np.float64), s32, b32))


@pytest.mark.parametrize("code", [0, 1, 2])
def test_float_image_generator(code):
    """the generator the GPU tests use: bytes follow the source image for f32 / f16, and the 1 % condition holds"""
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (9, 65, 4), dtype=np.uint8)
    el, by = float_image(img, code, [255.0] * 4, [0.0] * 4, rng)
    assert el.shape == by.shape == img.shape and by.dtype == np.uint8
    diff = np.abs(by.astype(int) - img.astype(int))
    if code == 0:
        assert (diff == 0).mean() > 0.99  # |d| < 0.45 never crosses a half (the few resampled elements may have a new byte)
    elif code == 1:
        assert (diff == 0).mean() > 0.9 and (diff <= 1).mean() > 0.99  # + f16's rounding, up to 0.06 of a byte
    else:
        assert (diff <= 1).mean() > 0.99  # bf16's step near 1.0 is a whole byte


# ---- subnormal source elements: widen_f16's host branch for them, the hardware conversion on the device ----
def subnormal_image(code, w, h, c):
    """-> (elements (h, w, c), scale[4], bias[4], the bytes by the rule).  Every element is a SUBNORMAL of its type, so every place
    of the image -- a row's first and last pixel, window interiors -- holds one, with a scale that brings them into the byte range:
    f16 (code 1): all 2046 non-zero subnormal bit patterns +-k * 2^-24, k = 1 ... 1023, scale 2^22 -- values +-k / 4, ties at
    k = 2 mod 4; f32 (code 0): +-k * 2^-149 for k on a stride through 1 ... 2^23 - 1 and next to 2^21 and 3 * 2^21, scale 2^127 --
    values +-k * 2^-22, exact ties at 0.5 and 1.5.  Products are exact in fp32 and in float64, so the rule's bytes are exact.  (bf16
    shares fp32's exponent range and widens by a shift: no case of its own.)  A flush of the source to zero gives all-zero bytes."""
    n = w * h * c
    i = np.arange(n, dtype=np.int64)
    if code == 1:
        pat = np.concatenate([np.arange(1, 1024), 0x8000 + np.arange(1, 1024)]).astype(np.uint16)
        assert pat.size == 2046 and n >= 2046
        el = pat[(i * 5 + i // (w * c)) % 2046].view(np.float16)  # (5 and 2046 are coprime: every pattern occurs; rows start apart)
        scale = 2.0 ** 22
    else:
        assert code == 0
        ks = np.concatenate([np.arange(1, 1 << 23, 4099), [(1 << 23) - 1], [m * (1 << 21) + d for m in (1, 3) for d in (-1, 0, 1)]]).astype(np.uint32)
        pat = np.concatenate([ks, ks[::3] | np.uint32(0x80000000)])
        assert n >= pat.size
        el = pat[(i * 7 + i // (w * c)) % pat.size].view(np.float32)
        scale = 2.0 ** 127
    el = el.reshape(h, w, c)
    x = element_values(el, code)
    assert bool(((x != 0) & (np.abs(x) < (2.0 ** -14 if code == 1 else 2.0 ** -126))).all())
    sc, bi = np.full(4, scale, dtype=np.float32), np.zeros(4, dtype=np.float32)
    by = oracle_quantize(x, sc[0], bi[0])
    return el, sc, bi, by


@pytest.mark.parametrize("code", [0, 1])
def test_subnormal_sources(built_lib, code):
    """fpng_amd_quantize_float on subnormal elements (f16: widen_f16's branch for a zero exponent; f32: no flush): the rule's
    bytes, ties to even among them, and the patterns the generator promises"""
    el, sc, bi, by = subnormal_image(code, 300, 9, 3)
    bits = np.ascontiguousarray(el).view(np.uint16 if code == 1 else np.uint32)
    if code == 1:
        assert np.unique(bits).size == 2046
        assert sorted(np.unique(by).tolist()) == list(range(256))
        k = np.arange(1, 1024)
        want = np.clip(np.rint(k / 4.0), 0, 255).astype(np.uint8)
        assert np.array_equal(lib_quantize(k.astype(np.uint16).view(np.float16), 1, sc[0], 0.0), want)
        assert want[1] == 0 and want[5] == 2 and want[9] == 2 and want[13] == 4  # k = 2, 6, 10, 14: 0.5, 1.5, 2.5, 3.5 to even
    else:
        assert sorted(np.unique(by).tolist()) == [0, 1, 2]
        ties = np.array([(1 << 21) - 1, 1 << 21, (1 << 21) + 1, 3 * (1 << 21) - 1, 3 * (1 << 21), 3 * (1 << 21) + 1], dtype=np.uint32).view(np.float32)
        assert lib_quantize(ties, 0, sc[0], 0.0).tolist() == [0, 0, 1, 1, 2, 2]
        assert set(ties.view(np.uint32).tolist()) <= set(bits.reshape(-1).tolist())
    assert np.array_equal(lib_quantize(el, code, sc[0], bi[0]), by)
    assert np.array_equal(lib_quantize(el[::-1, ::-1], code, sc[0], bi[0]), by[::-1, ::-1])
