"""GPU decoder into planar images of normalised floats (-m gpu; fpng_amd_decode_batch_planar_float /
fpng_amd_decode_batch_device_planar_float, dec_unfilter_float_kernel and dec_stored_float_kernel): three and four planes of f32,
f16 and bf16, every pitch kind, host and device files.

Expected values never come from the code under test: the pixels are the REFERENCE's decoder's (judge()), and an element is looked up
in a 256-entry table per channel, np.float32(np.float64(v) * np.float64(scale32) + np.float64(bias32)) -- the table builder checks
with fractions.Fraction that the float64 product and sum are EXACT, so their one rounding to float32 is what a single fp32 fused
multiply-add gives -- then torch's CPU conversion to f16 / bf16 (round to nearest even).  Buffers are compared whole and bitwise.
CONSTS are the constants a loader uses (results in [-2.2, 2.7]: no tie, subnormal or infinity); HARD are the ones at which the
rule's rounding, subnormals, overflow and zero sign show (test_float_cpu.py: which wrong epilogue each set tells from the rule)."""
import os
import struct
from fractions import Fraction

import numpy as np
import pytest

from cpu_ref import oracle
from test_gpu_decode import UNDECIDED, _device_files, judge
from test_gpu_decode_layouts import SENTINEL, _damaged_files, _encode_gpu, _header_dims, _matrix_files
from test_gpu_decode_planar import KINDS, _Region, _regions
import verify_files as vf

pytestmark = pytest.mark.gpu

DTYPES = ["float32", "float16", "bfloat16"]
ELEM = {"float32": 4, "float16": 2, "bfloat16": 2}


def _f32(values):
    return np.asarray(values, dtype=np.float64).astype(np.float32)


# (scale[4], bias[4]) as float32: ImageNet's mean / std with alpha 0.5 / 0.25; plain [0, 1]; [-1, 1]
_MEAN, _STD = (0.485, 0.456, 0.406, 0.5), (0.229, 0.224, 0.225, 0.25)
CONSTS = [(_f32([1.0 / (255.0 * s) for s in _STD]), _f32([-m / s for m, s in zip(_MEAN, _STD)])),
          (_f32([1.0 / 255.0] * 4), _f32([0.0] * 4)),
          (_f32([2.0 / 255.0] * 4), _f32([-1.0] * 4))]
# Constants at which the results ROUND HARD or leave a type's normal range -- CONSTS' 3 x 4 x 256 results lie in [-2.2, 2.7] and hold
# no f16 or bf16 tie, no subnormal of any type, no infinity and no -0.0.  Every value is an exact float32, the float64 product and
# sum are exact for all of them (test_float_cpu.py asserts both, and what each set holds), and no result is NaN.
HARD = {
    "A": (_f32([1.0, 1.0, 0.5, 2.0]), _f32([256.0, -511.0, 128.0, 512.0])),                           # bf16 ties
    "B": (_f32([1.0, 8.0, -257.0, 300.0]), _f32([2048.0, -4096.0, 0.0, -100.0])),                     # f16 ties, f16 overflow
    "C": (_f32([2.0 ** -24, 2.0 ** -25, -(2.0 ** -26), 3 * 2.0 ** -27]), _f32([0.0, 0.0, -0.0, 2.0 ** -24])),  # f16 subnormals, -0.0
    "D": (_f32([2.0 ** -149, -(2.0 ** -140), 0.0, -0.0]), _f32([0.0, 2.0 ** -133, -0.0, 0.0])),       # fp32 subnormals
    "E": (_f32([2.0 ** 127, -(2.0 ** 127), 2.0 ** 120, 2.0 ** 104]), _f32([0.0, 2.0 ** 127, 1.5 * 2.0 ** 127, -(2.0 ** 127)])),  # fp32 overflow
}


def _tables(consts, dtype):
    """table[c][v] = the BITS (uint32 / uint16) of round_to_dtype(fmaf(v, scale[c], bias[c])), without an fma: see the module docstring"""
    import torch
    scale, bias = consts
    f32 = np.empty((4, 256), dtype=np.float32)
    for c in range(4):
        s64, b64 = np.float64(scale[c]), np.float64(bias[c])
        for v in range(256):
            x = np.float64(v) * s64 + b64
            assert Fraction(float(x)) == Fraction(v) * Fraction(float(s64)) + Fraction(float(b64)), (c, v)  # the float64 value is exact
            with np.errstate(over="ignore"):  # (past float32's range: the infinity an fp32 fma gives)
                f32[c, v] = np.float32(x)
    if dtype == "float32":
        return f32.view(np.uint32)
    t = torch.from_numpy(f32).to(getattr(torch, dtype))
    return t.view(torch.int16).numpy().view(np.uint16)


def _sentinel(dtype):
    return np.uint32(0xA5A5A5A5) if dtype == "float32" else np.uint16(0xA5A5)


def _bits(px, tab):
    """(h, w, c) pixels -> (h, w, c) element bits"""
    return np.stack([tab[ch][px[:, :, ch]] for ch in range(px.shape[2])], axis=2)


@pytest.fixture(scope="module")
def enc(built_lib):
    import torch
    import fpng_amd
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    e = fpng_amd.Encoder(device=0)
    yield e
    e.close()


def _decode_float(enc, pngs, regs, total, dtype, consts, device):
    """one call into ONE sentinel-filled buffer of `total` elements: (results, the buffer's elements' bits afterwards, the views).
    The regions of test_gpu_decode_planar count ELEMENTS here: an odd pitch is an odd element pitch from an odd element offset."""
    import torch
    e = ELEM[dtype]
    buf = torch.full((total * e,), SENTINEL, dtype=torch.uint8, device="cuda")
    typed = buf.view(getattr(torch, dtype))
    views = [typed.as_strided((r.c, r.h, r.w), (r.pp, r.rp, 1), r.lo) for r in regs]
    orders, ups = [r.order() for r in regs], [r.kind == "bottom_up" for r in regs]
    if device:
        got = enc.decode_device_float(_device_files(pngs, shift=1), views, orders, ups, scale=consts[0], bias=consts[1])
    else:
        got = enc.decode_batch_float(pngs, views, orders, ups, scale=consts[0], bias=consts[1])
    torch.cuda.synchronize()
    return got, buf.cpu().numpy().view(np.uint32 if e == 4 else np.uint16), views


def _outside_untouched(host, regs, dtype):
    mask = np.ones(host.size, dtype=bool)
    for r in regs:
        for a, b in r.spans():
            mask[a:b] = False
    return bool(np.all(host[mask] == _sentinel(dtype)))


@pytest.fixture(scope="module")
def matrix(enc):
    pngs = _matrix_files(enc)
    judged = {d: [judge(p, d) for p in pngs] for d in (3, 4)}
    packed = {d: enc.decode_batch(pngs, d) for d in (3, 4)}
    return pngs, judged, packed


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", [3, 4])
def test_every_dtype_pitch_and_width(enc, matrix, c, dtype, device):
    """3- and 4-channel files x 1-pass, 2-pass and stored x widths around the epilogue's edges (1 ... 257, 7680) x heights around the
    48-row segment x pitch kinds dealt round-robin (tight, odd element pitch from an odd element offset, padded, bottom-up, reversed
    planes), into three and four planes of every dtype, one call per case into ONE buffer that is compared WHOLE: the expected bits
    in every span, the sentinel everywhere else.  The constant sets rotate so that every dtype meets all three."""
    pngs, judged, packed = matrix
    consts = CONSTS[((c - 3) * 2 + int(device) + DTYPES.index(dtype)) % 3]
    tab = _tables(consts, dtype)
    dims = [struct.unpack(">II", bytes(p[16:24])) for p in pngs]
    kinds = [KINDS[i % len(KINDS)] for i in range(len(pngs))]
    regs, total = _regions(dims, c, kinds)
    got, host, views = _decode_float(enc, pngs, regs, total, dtype, consts, device)
    exp = np.full(total, _sentinel(dtype), dtype=host.dtype)
    for i, (png, r, (st, view, cf)) in enumerate(zip(pngs, regs, got)):
        cst, cpx, w, h, fc = judged[c][i]
        pst, _, pcf = packed[c][i]
        assert st == cst == pst == 0 and cf == fc == pcf, (i, st, cst, pst)
        assert view is views[i]
        r.put(exp, _bits(np.asarray(cpx)[: w * h * c].reshape(h, w, c), tab))
    bad = np.nonzero(host != exp)[0]
    assert bad.size == 0, (c, dtype, device, bad.size, int(bad[0]), hex(int(host[bad[0]])), hex(int(exp[bad[0]])),
                           [(i, r.w, r.h, r.kind, int(bad[0]) - r.lo) for i, r in enumerate(regs) if r.off <= bad[0] < r.off + r.size])


_HARD_FILES = None


def hard_files():
    """(pngs, judged[desired][i]) -- made once, shared with test_gpu_decode_crop -- of the files the hard constant sets are decoded
    from: 3 and 4 channels x widths 257 ... 260 (a ragged row end of 1, 2, 3 and 0 elements behind the last whole quad) x 256 rows,
    pixel (x + 5 y + 64 ch) & 255, written 1-pass, 2-pass and stored by the oracle; the pixels are the reference's decoder's.
    Asserted on those pixels, not assumed: in every file every plane of the file's meets every byte value at every x mod 4 (a
    lane's quad) AND at every element of the last quad, so every table entry passes through every conversion site."""
    global _HARD_FILES
    if _HARD_FILES is None:
        pngs, chans = [], []
        for c in (3, 4):
            for w in (257, 258, 259, 260):
                y, x, ch = np.meshgrid(np.arange(256), np.arange(w), np.arange(c), indexing="ij")
                img = np.ascontiguousarray(((x + 5 * y + 64 * ch) & 255).astype(np.uint8))
                for fl in (0, 1, 2):
                    pngs.append(oracle().encode(img, w, 256, c, fl))
                    chans.append(c)
        assert [(p[60] & 6) != 0 for p in pngs] == [fl != 2 for _ in range(8) for fl in (0, 1, 2)]  # Deflate blocks, but for the stored ones
        judged = {d: [judge(p, d) for p in pngs] for d in (3, 4)}
        for d in (3, 4):
            for (st, px, w, h, fc), c in zip(judged[d], chans):
                assert st == 0 and h == 256 and fc == c
                px = np.asarray(px)[: w * h * d].reshape(h, w, d)
                last = (w - 1) & ~3
                for ch in range(d):
                    if ch >= c:
                        assert bool((px[:, :, ch] == 255).all())  # (the alpha a 3-channel file gets: scale[3] and bias[3] at 255)
                        continue
                    for k in range(4):
                        assert np.unique(px[:, k::4, ch]).size == 256, (w, c, ch, k)
                    for x in range(last, w):
                        assert np.unique(px[:, x, ch]).size == 256, (w, c, ch, x)
        _HARD_FILES = (pngs, judged)
    return _HARD_FILES


def _hard_case(enc, name, dtype, c, device, shift):
    """the hard files into c planes of `dtype` under HARD[name], pitch kinds dealt round-robin from `shift`: the whole buffer
    against the table look-up of the reference's pixels and the sentinel"""
    pngs, judged = hard_files()
    consts = HARD[name]
    tab = _tables(consts, dtype)
    dims = [struct.unpack(">II", bytes(p[16:24])) for p in pngs]
    kinds = [KINDS[(i + shift) % len(KINDS)] for i in range(len(pngs))]
    regs, total = _regions(dims, c, kinds)
    got, host, views = _decode_float(enc, pngs, regs, total, dtype, consts, device)
    exp = np.full(total, _sentinel(dtype), dtype=host.dtype)
    for i, (r, (st, view, cf)) in enumerate(zip(regs, got)):
        cst, cpx, w, h, fc = judged[c][i]
        assert st == cst == 0 and cf == fc and view is views[i], (i, st, cst)
        r.put(exp, _bits(np.asarray(cpx)[: w * h * c].reshape(h, w, c), tab))
    bad = np.nonzero(host != exp)[0]
    assert bad.size == 0, (name, c, dtype, device, bad.size, int(bad[0]), hex(int(host[bad[0]])), hex(int(exp[bad[0]])),
                           [(i, r.w, r.h, r.kind, int(bad[0]) - r.lo) for i, r in enumerate(regs) if r.off <= bad[0] < r.off + r.size])


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", sorted(HARD))
def test_hard_constants(enc, name, dtype, device):
    """Every set of HARD (bf16 ties; f16 ties and overflow; f16 subnormals and -0.0; fp32 subnormals; fp32 overflow) x every dtype
    x both entry points, into three and into four planes (a 3-channel file into four pins fmaf(255, scale[3], bias[3])): one fp32
    fused multiply-add, then round to nearest even -- ties to even, subnormal results kept, infinities past the type's range, the
    zero's sign -- bit for bit, at whole-quad stores, single-element stores at ragged row ends and the stored files' scalar path."""
    for c in (3, 4):
        _hard_case(enc, name, dtype, c, device, shift=sorted(HARD).index(name) + DTYPES.index(dtype) + c)


@pytest.mark.parametrize("dtype", DTYPES)
def test_hard_constants_with_checksums_verified(enc, dtype):
    """the subnormal sets (C: f16, D: fp32) through the kernels' verify instantiations (set_decode_verify(CRC | ADLER))"""
    enc.set_decode_verify(3)
    try:
        for k, name in enumerate(("C", "D")):
            for c in (3, 4):
                _hard_case(enc, name, dtype, c, device=bool((k + c) & 1), shift=k + c)
    finally:
        enc.set_decode_verify(0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_constants_belong_to_file_channels(enc, dtype):
    """Three (four) different scales: planes stored in reverse get, per FILE channel, the values that forward planes get; and
    mean / std through the Python door is torchvision's Normalize on [0, 1] values up to the constants' and the result's rounding."""
    import torch
    import fpng_amd
    tdt = getattr(torch, dtype)
    consts = CONSTS[0]
    tab = _tables(consts, dtype)
    items = [(fpng_amd.synth_image("noise", 65, 49, 4, seed=1), 0), (fpng_amd.synth_image("grad", 257, 5, 3, seed=2), 1),
             (fpng_amd.synth_image("noise", 31, 3, 3, seed=3), 2)]
    pngs = _encode_gpu(enc, items)
    for png, (img, _) in zip(pngs, items):
        h, w, fc = img.shape
        for c in (3, 4):
            cst, cpx, *_ = judge(png, c)
            want = _bits(np.asarray(cpx)[: w * h * c].reshape(h, w, c), tab).transpose(2, 0, 1)
            fwd = torch.zeros((c, h, w), dtype=tdt, device="cuda")
            rev = torch.zeros((c, h, w), dtype=tdt, device="cuda")
            (st, v, cf), = enc.decode_batch_float([png], [fwd], scale=consts[0], bias=consts[1])
            assert st == 0 and v is fwd and cf == fc
            (st, v, cf), = enc.decode_device_float(_device_files([png]), [rev], "bgr" if c == 3 else "abgr", scale=consts[0], bias=consts[1])
            assert st == 0 and v is rev
            ibits = torch.int32 if dtype == "float32" else torch.int16
            got = fwd.view(ibits).cpu().numpy().view(want.dtype)
            assert np.array_equal(got, want), (w, h, c)
            assert torch.equal(rev.flip(0).view(ibits), fwd.view(ibits)), (w, h, c)
            # the door's mean / std form: the same constants, so the same bits; and what Normalize computes, within rounding
            out = torch.zeros((c, h, w), dtype=tdt, device="cuda")
            (st, _, _), = enc.decode_batch_float([png], [out], mean=_MEAN[:c], std=_STD[:c])
            assert st == 0 and torch.equal(out.view(ibits), fwd.view(ibits))
            px = torch.from_numpy(np.asarray(cpx)[: w * h * c].reshape(h, w, c).astype(np.float64)).permute(2, 0, 1)
            ref = (px / 255.0 - torch.tensor(_MEAN[:c], dtype=torch.float64)[:, None, None]) / torch.tensor(_STD[:c], dtype=torch.float64)[:, None, None]
            # float32: |v * scale| < 4.5 and |bias| < 2.2 carry their constants' rounding, the result (< 2.7) its own: 9.4 * 2^-24 < 6e-7;
            # f16 / bf16 add half an ulp of the result: 2^-11 / 2^-8 relative
            rel = {"float32": 0.0, "float16": 2.0 ** -11, "bfloat16": 2.0 ** -8}[dtype]
            assert bool(((out.cpu().double() - ref).abs() <= 6e-7 + rel * ref.abs()).all()), (w, h, c)


@pytest.mark.parametrize("device", [False, True])
def test_damaged_and_undecided_files_write_nothing_outside_the_spans(enc, device):
    """container_mutator / token_mutator files, and every compressed file UNDECIDED (FPNG_AMD_DECODE_MAX_ROUNDS=0): each status and
    channels_in_file is the packed call's at the same desired channels, and every element outside the spans keeps its sentinel."""
    pngs = _damaged_files()
    dims = [_header_dims(p) for p in pngs]
    kinds = [KINDS[i % len(KINDS)] for i in range(len(pngs))]
    for c in (3, 4):
        for forced in (False, True):
            dtype = DTYPES[(c + int(forced) + int(device)) % 3]
            if forced:
                os.environ["FPNG_AMD_DECODE_MAX_ROUNDS"] = "0"
            try:
                packed = enc.decode_batch(pngs, c)
                regs, total = _regions(dims, c, kinds)
                got, host, _ = _decode_float(enc, pngs, regs, total, dtype, CONSTS[0], device)
            finally:
                if forced:
                    del os.environ["FPNG_AMD_DECODE_MAX_ROUNDS"]
            sts = [st for st, _, _ in got]
            assert sts == [st for st, _, _ in packed], (c, forced, dtype)
            assert [cf for _, _, cf in got] == [cf for _, _, cf in packed], (c, forced, dtype)
            if forced:
                assert UNDECIDED in sts
            assert any(st not in (0, UNDECIDED) for st in sts)
            assert _outside_untouched(host, regs, dtype), (c, forced, device, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_checksums_are_verified(enc, dtype):
    """set_decode_verify(3): good files (compressed and stored) decode to the same bits as without the check; a flipped CRC byte
    returns 65, a wrong Adler-32 (CRC recomputed) 66."""
    import fpng_amd
    items = [(fpng_amd.synth_image("blocks", 257, 49, 4, seed=5), 0), (fpng_amd.synth_image("grad", 65, 97, 3, seed=6), 1),
             (fpng_amd.synth_image("noise", 63, 47, 4, seed=7), 2)]
    good = [bytes(p) for p in _encode_gpu(enc, items)]
    dims = [(im.shape[1], im.shape[0]) for im, _ in items]
    bad = [vf.flip_crc_bit(good[0]), vf.with_adler(good[0], vf.stored_adler(good[0]) ^ 0x100), vf.with_adler(good[2], vf.stored_adler(good[2]) ^ 1),
           vf.flip_crc_bit(good[1], bit=17)]
    bad_dims = [dims[0], dims[0], dims[2], dims[1]]
    kinds = ["odd", "bottom_up", "reversed", "packed", "pad256", "odd", "reversed"]
    for device in (False, True):
        regs, total = _regions(dims, 4, kinds)
        plain, host0, _ = _decode_float(enc, good, regs, total, dtype, CONSTS[0], device)
        assert [st for st, _, _ in plain] == [0, 0, 0]
        enc.set_decode_verify(3)
        try:
            checked, host1, _ = _decode_float(enc, good, regs, total, dtype, CONSTS[0], device)
            regs_b, total_b = _regions(dims + bad_dims, 3, kinds)
            got, host_b, _ = _decode_float(enc, good + bad, regs_b, total_b, dtype, CONSTS[0], device)
        finally:
            enc.set_decode_verify(0)
        assert [st for st, _, _ in checked] == [0, 0, 0] and np.array_equal(host0, host1), device
        assert [st for st, _, _ in got] == [0, 0, 0, 65, 66, 66, 65], device
        assert [vf.expected_status(p, 3) for p in bad] == [65, 66, 66, 65]  # (zlib agrees)
        assert _outside_untouched(host_b, regs_b, dtype)


def _raw_call(enc, pngs, recs, fmt, device):
    """fpng_amd_decode_batch(_device)_planar_float on hand-made records (num_chans, d_pixels, row_pitch, plane_pitch, cap) and a
    hand-made format (dtype, reserved, scale[4], bias[4]): (rc, statuses)"""
    import torch
    import ctypes as C
    from fpng_amd import _lib
    n = len(recs)
    arr = (_lib.PngPlanarIn * n)()
    res = (_lib.DecodeResult * n)()
    f = _lib.FloatFormat()
    f.dtype, f.reserved = fmt[0], fmt[1]
    for k in range(4):
        f.scale[k], f.bias[k] = fmt[2][k], fmt[3][k]
    keep = _device_files(pngs, shift=1) if device else [np.frombuffer(bytes(p), dtype=np.uint8) for p in pngs]
    for i, (c, ptr, rp, pp, cap) in enumerate(recs):
        arr[i].data = keep[i].data_ptr() if device else keep[i].ctypes.data
        arr[i].size = len(pngs[i])
        arr[i].num_chans, arr[i].d_pixels, arr[i].row_pitch, arr[i].plane_pitch, arr[i].pixels_cap = c, ptr, rp, pp, cap
    fn = enc.lib.fpng_amd_decode_batch_device_planar_float if device else enc.lib.fpng_amd_decode_batch_planar_float
    enc._sync_stream()
    rc = fn(enc.h, arr, n, C.byref(f), res)
    torch.cuda.synchronize()
    return rc, [r.status for r in res]


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_validation(enc, dtype, device):
    """Every rule gets its error code, the call writes nothing (the sentinel-filled buffer stays as it was -- also the valid file's
    part in front of the bad one), and the next valid call -- exact cap, odd element offset and pitches, negative pitches -- succeeds."""
    import torch
    INVALID, SMALL = -1, -4
    e, code = ELEM[dtype], DTYPES.index(dtype)
    w, h = 37, 21
    good = _encode_gpu(enc, [(np.random.default_rng(3).integers(0, 256, (h, w, 4), dtype=np.uint8), 0)])[0]
    buf = torch.full((1 << 17,), SENTINEL, dtype=torch.uint8, device="cuda")
    base = buf.data_ptr()
    one, zero = [1.0 / 255.0] * 4, [0.0] * 4
    fmt = (code, 0, one, zero)
    full = (3 * w * h + (h - 1) * w + w) * e  # span of four tight planes, in bytes
    ok = (4, base, 0, 0, full)
    far = base + 32768
    rp, pp = (w + 3) * e, (h * (w + 3) + 1) * e
    span3 = 2 * pp + (h - 1) * rp + w * e
    inf, nan = float("inf"), float("nan")
    cases = [
        ((4, far + e // 2, 0, 0, 1 << 15), fmt, INVALID),                       # a base that is no multiple of the element size
        ((4, far + 1, 0, 0, 1 << 15), fmt, INVALID),
        ((3, far, rp + 1, pp, 1 << 15), fmt, INVALID),                          # ... a row pitch
        ((3, far, rp, pp + e // 2, 1 << 15), fmt, INVALID),                     # ... a plane pitch
        ((3, far + 2 * pp, rp, -(pp + 1), 1 << 15), fmt, INVALID),
        (ok, (3, 0, one, zero), INVALID),                                      # dtype
        (ok, (code, 1, one, zero), INVALID),                                   # reserved
        (ok, (code, 0, [1.0, inf, 1.0, 1.0], zero), INVALID),                  # a scale or bias that is not finite
        (ok, (code, 0, one, [0.0, 0.0, 0.0, nan]), INVALID),
        (ok, (code, 0, [-inf, 1.0, 1.0, 1.0], zero), INVALID),
        ((4, far, (w - 1) * e, 0, 1 << 15), fmt, INVALID),                      # |row_pitch| < w elements
        ((4, far, w * e, (h * w - 1) * e, 1 << 15), fmt, INVALID),              # planes overlap
        ((5, far, 0, 0, 1 << 15), fmt, INVALID),                                # num_chans
        ((4, far, 0, 0, full - 1), fmt, SMALL),                                 # cap one byte short
        ((3, far + e, rp, pp, span3 - 1), fmt, SMALL),
        ((4, 0, 0, 0, 1 << 15), fmt, SMALL),                                    # no buffer
    ]
    for rec, f, want in cases:
        rc, _ = _raw_call(enc, [good, good], [ok, rec], f, device)
        assert rc == want, (rec, f, rc)
        assert bool((buf == SENTINEL).all()), (rec, f)
    o3, o4 = 32768 + e, 65536
    rc, sts = _raw_call(enc, [good, good, good], [ok, (3, base + o3, rp, pp, span3), (4, base + o4 + (3 * h * w + (h - 1) * w) * e, -w * e, -h * w * e, full)], fmt, device)
    assert rc == 0 and sts == [0, 0, 0], (rc, sts)
    tab = _tables((_f32(one), _f32(zero)), dtype)
    cst, cpx, *_ = judge(good, 4)
    px = _bits(np.asarray(cpx)[: w * h * 4].reshape(h, w, 4), tab)
    host = buf.cpu().numpy().view(tab.dtype)
    exp = np.full(host.size, _sentinel(dtype), dtype=tab.dtype)
    exp[: 4 * h * w] = px.transpose(2, 0, 1).reshape(-1)
    for ch in range(3):
        for y in range(h):
            a = (o3 + ch * pp + y * rp) // e
            exp[a: a + w] = px[y, :, ch]
    exp[o4 // e: o4 // e + 4 * h * w] = px.transpose(2, 0, 1)[::-1, ::-1].reshape(-1)  # planes A,B,G,R, rows bottom-up
    assert np.array_equal(host, exp)
