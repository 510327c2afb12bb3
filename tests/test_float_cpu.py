"""No-GPU tests of the float decode interface (fpng_amd_decode_batch(_device)_planar_float): the two exported entry points and the
fpng_amd_float_format record, normalize_constants, dest_layout_float on CPU tensor views of the three dtypes (it only reads strides
and data_ptr()), and the descriptor make_decode_batch_float builds: byte pitches and pixels_cap from strides in elements."""
import ctypes as C

import numpy as np
import pytest
import torch

import fpng_amd
from fpng_amd import _lib
from fpng_amd.api import Encoder, dest_layout_float, dest_layout_planar, normalize_constants

DTYPES = [(torch.float32, 4, 0), (torch.float16, 2, 1), (torch.bfloat16, 2, 2)]


def test_entry_points_and_record(built_lib):
    lib = _lib.load()
    for name in ("fpng_amd_decode_batch_planar_float", "fpng_amd_decode_batch_device_planar_float"):
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None
    assert lib.fpng_amd_abi_version() == 5  # (new entry points, the same ABI version)
    assert C.sizeof(_lib.FloatFormat) == 40
    offs = {n: getattr(_lib.FloatFormat, n).offset for n, _ in _lib.FloatFormat._fields_}
    assert offs == {"dtype": 0, "reserved": 4, "scale": 8, "bias": 24}
    assert (_lib.F32, _lib.F16, _lib.BF16) == (0, 1, 2)
    assert fpng_amd.FLOAT_DTYPES == {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}


def test_null_arguments_are_refused_without_a_device(built_lib):
    lib = _lib.load()
    fmt = _lib.FloatFormat()
    for fn in (lib.fpng_amd_decode_batch_planar_float, lib.fpng_amd_decode_batch_device_planar_float):
        assert fn(None, None, 1, C.byref(fmt), None) == -1
        assert fn(None, None, 1, None, None) == -1


def test_normalize_constants():
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    scale, bias = normalize_constants(mean, std)
    assert scale.dtype == bias.dtype == np.float32 and scale.shape == bias.shape == (4,)
    for c in range(3):
        assert scale[c] == np.float32(1.0 / (255.0 * std[c])) and bias[c] == np.float32(-mean[c] / std[c])
    assert scale[3] == np.float32(1.0 / 255.0) and bias[3] == 0.0  # (missing channels: plain [0, 1])
    scale, bias = normalize_constants(mean + (0.5,), std + (0.25,))
    assert scale[3] == np.float32(1.0 / (255.0 * 0.25)) and bias[3] == np.float32(-2.0)
    scale, bias = normalize_constants([0.5], [0.5], max_value=1.0)
    assert list(scale) == [2.0, 1.0, 1.0, 1.0] and list(bias) == [-1.0, 0.0, 0.0, 0.0]
    scale, bias = normalize_constants([], [])
    assert np.all(scale == np.float32(1.0 / 255.0)) and np.all(bias == 0)
    for bad in (((0.5, 0.5), (0.5,)), ((0.5,) * 5, (0.5,) * 5), ((0.5,), (0.0,)), ((float("nan"),), (1.0,)), ((0.5,), (float("inf"),))):
        with pytest.raises(ValueError):
            normalize_constants(*bad)
    with pytest.raises(ValueError):
        normalize_constants([0.5], [0.5], max_value=0.0)


@pytest.mark.parametrize("dtype,e,code", DTYPES)
def test_dest_layout_float(dtype, e, code):
    """the uint8 rules on strides counted in elements; pitches and pointer offsets in bytes"""
    for c, h, w in ((3, 5, 7), (4, 5, 7), (3, 1, 9), (4, 9, 1), (3, 1, 1)):
        t = torch.zeros(c, h, w, dtype=dtype)
        assert dest_layout_float(t) == (t.data_ptr(), (w * e if h > 1 else 0), h * w * e, code)  # (one row: no pitch, the C side takes w * e)
    n = torch.zeros(5, 3, 6, 11, dtype=dtype)
    assert dest_layout_float(n[2]) == (n.data_ptr() + 2 * 3 * 66 * e, 11 * e, 66 * e, code)
    q = torch.zeros(4, 6, 11, dtype=dtype)
    assert dest_layout_float(q[:3]) == (q.data_ptr(), 11 * e, 66 * e, code)
    t = torch.zeros(3, 40, 50, dtype=dtype)
    assert dest_layout_float(t[:, 7:19, 3:44]) == (t.data_ptr() + (7 * 50 + 3) * e, 50 * e, 2000 * e, code)  # a crop
    assert dest_layout_float(t[:, 7:8, 3:44]) == (t.data_ptr() + (7 * 50 + 3) * e, 0, 2000 * e, code)  # ... of one row
    buf = torch.zeros(4, 10, 64, dtype=dtype)
    assert dest_layout_float(buf[:, :, :33]) == (buf.data_ptr(), 64 * e, 640 * e, code)  # padded rows
    t = torch.zeros(3, 6, 11, dtype=dtype)
    assert dest_layout_float(t, bottom_up=True) == (t.data_ptr() + 5 * 11 * e, -11 * e, 66 * e, code)
    assert dest_layout_float(t, order="bgr") == (t.data_ptr() + 2 * 66 * e, 11 * e, -66 * e, code)
    assert dest_layout_float(t, order="BGR", bottom_up=True) == (t.data_ptr() + (2 * 66 + 5 * 11) * e, -11 * e, -66 * e, code)
    assert dest_layout_float(q, order="abgr") == (q.data_ptr() + 3 * 66 * e, 11 * e, -66 * e, code)
    assert dest_layout_float(q, order="rgba") == dest_layout_float(q, order="rgb")
    one = torch.zeros(3, 1, 11, dtype=dtype)
    assert dest_layout_float(one, bottom_up=True) == (one.data_ptr(), 0, 11 * e, code)
    # the same view as bytes gives the same pointer and pitches
    assert dest_layout_float(t[:, 1:5, 2:9], "bgr", True)[:3] == dest_layout_planar(t[:, 1:5, 2:9].view(torch.uint8), "bgr", True)


@pytest.mark.parametrize("dtype,e,code", DTYPES)
def test_refusals(dtype, e, code):
    t = torch.zeros(3, 6, 11, dtype=dtype)
    q = torch.zeros(4, 6, 11, dtype=dtype)
    for bad in ("bgra", "argb", "bgr", "rgbx", "xyz"):
        with pytest.raises(ValueError):
            dest_layout_float(q, order=bad)
    for bad in ("rgba", "abgr", "rbg", ""):
        with pytest.raises(ValueError):
            dest_layout_float(t, order=bad)
    for other in (torch.uint8, torch.int8, torch.float64, torch.int32):
        with pytest.raises(ValueError):
            dest_layout_float(torch.zeros(3, 4, 5, dtype=other))
    for shape in ((2, 3, 4, 5), (4, 5), (2, 4, 5), (5, 4, 5)):  # rank, plane count
        with pytest.raises(ValueError):
            dest_layout_float(torch.zeros(*shape, dtype=dtype))
    with pytest.raises(ValueError):
        dest_layout_float("not a tensor")
    with pytest.raises(ValueError, match="decode_device_ex"):  # an interleaved view
        dest_layout_float(torch.zeros(6, 11, 3, dtype=dtype).permute(2, 0, 1))
    for view in (t[:, :, ::2], t[:1].expand(3, 6, 11), t[:, :1].expand(3, 6, 11), torch.as_strided(t, (3, 6, 11), (66, 10, 1)),
                 torch.as_strided(t, (3, 6, 11), (65, 11, 1)), torch.as_strided(t, (3, 6, 11), (11, 33, 1))):
        with pytest.raises(ValueError):
            dest_layout_float(view)
    assert dest_layout_float(torch.as_strided(t, (3, 5, 10), (66, 11, 1)))  # (the same with room: fine)


@pytest.mark.parametrize("dtype,e,code", DTYPES)
def test_make_decode_batch_float_on_cpu_tensors(dtype, e, code):
    big = torch.zeros(4, 20, 30, dtype=dtype)
    views = [big, big[:3, 2:12, 5:25], big[:3]]
    files = [b"\x89PNG", b"", b"abc"]
    d = Encoder.make_decode_batch_float(files, views, order=["rgba", "rgb", "bgr"], bottom_up=[False, True, False], mean=(0.5, 0.25, 0.125), std=(0.5, 0.25, 2.0))
    assert isinstance(d, fpng_amd.DecodeBatchFloat) and not isinstance(d, (fpng_amd.DecodeBatchEx, fpng_amd.DecodeBatchPlanar)) and not d.device_data
    assert (d.fmt.dtype, d.fmt.reserved) == (code, 0)
    sc, bi = normalize_constants((0.5, 0.25, 0.125), (0.5, 0.25, 2.0))
    assert list(d.fmt.scale) == [float(v) for v in sc] and list(d.fmt.bias) == [float(v) for v in bi]
    a = d.arr[0]
    assert (a.size, a.num_chans, a.d_pixels, a.row_pitch, a.plane_pitch, a.pixels_cap) == (4, 4, big.data_ptr(), 30 * e, 600 * e, (3 * 600 + 19 * 30 + 30) * e)
    a = d.arr[1]
    assert a.data is None and a.size == 0
    assert (a.num_chans, a.d_pixels, a.row_pitch, a.plane_pitch) == (3, big.data_ptr() + (2 * 30 + 5 + 9 * 30) * e, -30 * e, 600 * e)
    assert a.pixels_cap == (2 * 600 + 9 * 30 + 20) * e  # the view's own span, in bytes
    a = d.arr[2]
    assert (a.d_pixels, a.plane_pitch, a.pixels_cap) == (big.data_ptr() + 1200 * e, -600 * e, (2 * 600 + 19 * 30 + 30) * e)
    assert len(d.res) == 3 and list(d.statuses()) == [0, 0, 0]
    # scale / bias given directly, padded with 1 / 255 and 0; neither: plain [0, 1]
    d = Encoder.make_decode_batch_float(files[:1], views[:1], scale=[2.0 / 255.0] * 3, bias=[-1.0])
    assert list(d.fmt.scale) == [float(np.float32(2.0 / 255.0))] * 3 + [float(np.float32(1.0 / 255.0))] and list(d.fmt.bias) == [-1.0, 0.0, 0.0, 0.0]
    d = Encoder.make_decode_batch_float(files[:1], views[:1])
    assert list(d.fmt.scale) == [float(np.float32(1.0 / 255.0))] * 4 and list(d.fmt.bias) == [0.0] * 4
    for kw in (dict(mean=[0.5]), dict(std=[0.5]), dict(mean=[0.5], std=[0.5], scale=[1.0]), dict(scale=[float("inf")]), dict(bias=[float("nan")]),
               dict(scale=[1.0] * 5)):
        with pytest.raises(ValueError):
            Encoder.make_decode_batch_float(files[:1], views[:1], **kw)


def test_mixed_dtypes_are_refused():
    outs = [torch.zeros(3, 2, 2, dtype=torch.float32), torch.zeros(3, 2, 2, dtype=torch.float16)]
    with pytest.raises(ValueError, match="one dtype"):
        Encoder.make_decode_batch_float([b"x", b"y"], outs)
    with pytest.raises(ValueError):
        Encoder.make_decode_batch_float([b"x"], [torch.zeros(3, 2, 2, dtype=torch.uint8)])


def test_descriptors_of_the_other_kinds_are_refused(built_lib):
    """a float descriptor handed to the _ex and _planar calls, and theirs to the float calls: ValueError before any device call"""
    e = Encoder.__new__(Encoder)  # (no device: an encoder object without a handle)
    e.lib, e.h = _lib.load(), None
    flt = Encoder.make_decode_batch_float([b"x"], [torch.zeros(3, 2, 2, dtype=torch.float16)])
    for fn in (Encoder.decode_device_ex, Encoder.decode_batch_ex, Encoder.decode_device_planar, Encoder.decode_batch_planar):
        with pytest.raises(ValueError, match="float"):
            fn(e, flt)
    planar = Encoder.make_decode_batch_planar([b"x"], [torch.zeros(3, 2, 2, dtype=torch.uint8)])
    ex = fpng_amd.DecodeBatchEx([], [], None, None, False, [])
    for fn in (Encoder.decode_device_float, Encoder.decode_batch_float):
        for other in (planar, ex):
            with pytest.raises(ValueError, match="make_decode_batch_float"):
                fn(e, other)
    with pytest.raises(ValueError, match="host memory"):
        Encoder.decode_device_float(e, flt)  # (host files: decode_batch_float)
    with pytest.raises(ValueError, match="CUDA"):
        Encoder.decode_batch_float(e, flt)  # (CPU destinations)


# ---- the constant sets of the GPU tests: what they hold, and which wrong epilogues they tell from the rule ----
def _f16_of(f32, mode):
    """float32 values -> float16 bits by integer arithmetic: mode "even" (the rule), "away" (ties away from zero) or "trunc"
    (toward zero).  -> (bits, a mask of the finite values that lie exactly half way between two float16 values)"""
    x = np.abs(f32.astype(np.float64))
    finite = np.isfinite(x)
    _, e = np.frexp(np.where(finite & (x > 0), x, 1.0))  # x = m * 2^e, 0.5 <= m < 1
    q = np.ldexp(1.0, np.maximum(e - 1, -14) - 10)  # the float16 step at x (subnormals: 2^-24)
    n = np.where(finite, x, 0.0) / q  # exact: a power of two
    lo = np.floor(n)
    tie = finite & (n - lo == 0.5)
    up = {"even": (n - lo > 0.5) | (tie & (lo % 2 == 1)), "away": n - lo >= 0.5, "trunc": np.zeros(n.shape, dtype=bool)}[mode]
    r = (lo + up) * q
    big = r > 65504.0
    r = np.where(big, 65504.0 if mode == "trunc" else np.inf, r)
    r = np.where(finite, r, np.inf)
    bits = r.astype(np.float16).view(np.uint16)  # (exact: r is a float16 value)
    return bits | (f32.view(np.uint32) >> 16 & 0x8000).astype(np.uint16), tie & ~big | (tie & (x == 65520.0))


def _bf16_of(f32, mode):
    b = f32.view(np.uint32).astype(np.uint64)
    tie = np.isfinite(f32) & (b & 0xFFFF == 0x8000)
    add = 0x8000 if mode == "away" else 0x7FFF + (b >> 16 & 1)
    return ((b + add) >> 16).astype(np.uint16), tie


def _flush(bits, mant, exp):
    """subnormals of a bit pattern (mantissa mask, exponent mask) to a zero of their sign"""
    sub = (bits & exp == 0) & (bits & mant != 0)
    return np.where(sub, bits & ~np.array(mant | exp, dtype=bits.dtype), bits), sub


def _census(consts):
    """the reference tables of one constant set, what they hold, and which of the five wrong epilogues they show"""
    from test_gpu_decode_float import _tables
    scale, bias = consts
    assert scale.dtype == bias.dtype == np.float32 and scale.shape == bias.shape == (4,)
    t32 = _tables(consts, "float32")  # (asserts with fractions.Fraction that every float64 product and sum is exact)
    f32 = t32.view(np.float32)
    assert not np.isnan(f32).any()
    t16, tb = _tables(consts, "float16"), _tables(consts, "bfloat16")
    even16, tie16 = _f16_of(f32, "even")
    evenb, tieb = _bf16_of(f32, "even")
    # torch's conversions, numpy's and the integer models here are the same round-to-nearest-even
    with np.errstate(over="ignore"):
        assert np.array_equal(t16, f32.astype(np.float16).view(np.uint16)) and np.array_equal(t16, even16) and np.array_equal(tb, evenb)
    flushed32, sub32 = _flush(t32, 0x007FFFFF, 0x7F800000)
    flushed16, sub16 = _flush(t16, 0x03FF, 0x7C00)
    holds = {"bf16_ties": int(tieb.sum()), "f16_ties": int(tie16.sum()), "f16_inf": int((t16 & 0x7FFF == 0x7C00).sum()),
             "f16_subnormals": int(sub16.sum()), "f32_subnormals": int(sub32.sum()), "f32_inf": int(np.isinf(f32).sum()),
             "minus_zero": int((t32 == 0x80000000).sum())}
    wrong = {"bf16_half_away": int((_bf16_of(f32, "away")[0] != tb).sum()), "f16_half_away": int((_f16_of(f32, "away")[0] != t16).sum()),
             "f32_flushed": int((flushed32 != t32).sum()), "f16_flushed": int((flushed16 != t16).sum()),
             "f16_truncated": int((_f16_of(f32, "trunc")[0] != t16).sum())}
    return holds, wrong


# per set: what its tables must hold (counts of the 4 x 256 entries), and the wrong epilogues it is there to show
HARD_HOLDS = {
    "A": ({"bf16_ties": 512}, ["bf16_half_away"]),
    "B": ({"f16_ties": 190, "bf16_ties": 165, "f16_inf": 38}, ["f16_half_away", "bf16_half_away", "f16_truncated"]),
    "C": ({"f16_subnormals": 1018, "f16_ties": 224, "minus_zero": 1}, ["f16_flushed", "f16_half_away", "f16_truncated"]),
    "D": ({"f32_subnormals": 510}, ["f32_flushed"]),
    "E": ({"f32_inf": 699}, []),
}


def test_the_hard_constant_sets_tell_wrong_epilogues_from_the_rule():
    """test_gpu_decode_float.HARD, sets A-E, against five wrong models of the float epilogue: bf16 and f16 conversions that round
    half away from zero, fp32 and f16 results with subnormals flushed to zero, and an f16 conversion that truncates.  The three
    older sets (CONSTS: ImageNet's mean / std, 1 / 255, 2 / 255 - 1) show NONE of the first four -- asserted below -- because their
    tables hold no tie, no subnormal, no infinity and no -0.0; each of A-E must hold what it was written for (the counts, exactly)
    and show the models named with it, so a set that is edited, or replaced by one of the old three, fails here.  Also asserted, for
    every set: exact float32 constants, no NaN, and float64 arithmetic that is exact (so that _tables IS one fused multiply-add)."""
    from test_gpu_decode_float import CONSTS, HARD
    for k, consts in enumerate(CONSTS):
        holds, wrong = _census(consts)
        assert not any(holds.values()), (k, holds)
        assert [wrong[m] for m in ("bf16_half_away", "f16_half_away", "f32_flushed", "f16_flushed")] == [0] * 4 and wrong["f16_truncated"] > 400, (k, wrong)
    assert sorted(HARD) == sorted(HARD_HOLDS)
    seen = set()
    for name, consts in HARD.items():
        holds, wrong = _census(consts)
        want, shows = HARD_HOLDS[name]
        assert {key: holds[key] for key in want} == want, (name, holds)
        for m in shows:
            assert wrong[m] > 0, (name, m, wrong)
        seen |= {m for m, n in wrong.items() if n}
    assert seen == {"bf16_half_away", "f16_half_away", "f32_flushed", "f16_flushed", "f16_truncated"}
