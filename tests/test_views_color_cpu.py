"""No-GPU tests of the per-view colour matrix of the views calls (fpng_amd_decode_batch(_device)_planar_views_color /
_hwc_views_color): the host twin fpng_amd_color_apply -- the text the kernel runs -- against the exact model of color_model.py,
bit for bit; the model's array text against its integer text; every call-level refusal, none of which needs an encoder or a
device; color_matrix(); the color= keyword of the Python door."""
import ctypes as C

import numpy as np
import pytest
import torch

import fpng_amd
from fpng_amd import _lib
from fpng_amd.api import Encoder

import color_model as CM
from test_resize_view_cpu import BAD, GOOD

PLANAR = ("fpng_amd_decode_batch_planar_views_color", "fpng_amd_decode_batch_device_planar_views_color")
HWC = ("fpng_amd_decode_batch_hwc_views_color", "fpng_amd_decode_batch_device_hwc_views_color")
IDENTITY = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], dtype=np.float32)
# x.5 -> even (every odd byte is a tie); the clamp's two ends (4 x - 300 is below 0 up to 75 and above 255 from 139 on); channels
# mixed with both; the largest entries the call takes
TIES = np.array([[0.5, 0, 0, 0], [0, 0.5, 0, 0.5], [0, 0, 0.5, 1.0]], dtype=np.float32)
CLAMP_GAIN = np.array([[4, 0, 0, -300], [0, 4, 0, -300], [0, 0, 4, -300]], dtype=np.float32)
CLAMP_MIX = np.array([[4, 0, 0, 0], [-1, 0, 0, 64], [0.5, 0.5, 0.5, -300]], dtype=np.float32)
LARGEST = [np.full((3, 4), 65536.0, dtype=np.float32), np.full((3, 4), -65536.0, dtype=np.float32),
           np.array([[65536, -65536, 65536, -65536], [-65536, 65536, 0, 65536], [65536, 65536, -65536, -65536]], dtype=np.float32)]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _random_matrices(rng, n):
    ms = rng.uniform(-4.0, 4.0, size=(n, 3, 4))
    ms[:, :, 3] = rng.uniform(-300.0, 300.0, size=(n, 3))
    return ms.astype(np.float32)


def _model(m, px):
    return np.array([CM.apply(m, p) for p in px.reshape(-1, 3)], dtype=np.float32).reshape(px.shape)


def test_entry_points_and_record(built_lib):
    lib = _lib.load()
    for name in PLANAR + HWC + ("fpng_amd_color_apply",):
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
    assert lib.fpng_amd_abi_version() == 5  # (new entry points, the same ABI version)
    assert C.sizeof(_lib.ViewColor) == 64
    assert {n: getattr(_lib.ViewColor, n).offset for n, _ in _lib.ViewColor._fields_} == {"m": 0, "flags": 48, "reserved": 52}


def test_the_host_twin_is_the_model_on_random_pixels_and_matrices(built_lib):
    rng = np.random.default_rng(20)
    px = rng.integers(0, 256, size=(3000, 3), dtype=np.uint8)
    for m in _random_matrices(rng, 36):
        got = fpng_amd.color_apply(m, px)
        assert got.dtype == np.float32 and got.shape == px.shape
        assert np.array_equal(_bits(got), _bits(_model(m, px))), m
        assert np.array_equal(_bits(got), _bits(CM.apply_np(m, px))), m  # (the model's array text, which the GPU tests use)


def test_the_host_twin_on_the_identity_ties_clamps_and_the_largest_entries(built_lib):
    ramp = np.arange(256, dtype=np.uint8)
    every = np.stack([ramp, ramp[::-1], np.roll(ramp, 77)], axis=1)  # all 256 bytes in each channel
    got = fpng_amd.color_apply(IDENTITY, every)
    assert np.array_equal(_bits(got), _bits(every.astype(np.float32)))  # (exactly the byte, and +0.0 for 0)
    corners = np.array([[r, g, b] for r in (0, 1, 75, 76, 138, 139, 255) for g in (0, 127, 128, 255) for b in (0, 1, 254, 255)], dtype=np.uint8)
    for m in [TIES, CLAMP_GAIN, CLAMP_MIX] + LARGEST:
        for px in (every, corners):
            got = fpng_amd.color_apply(m, px)
            assert np.isfinite(got).all() and got.min() >= 0.0 and got.max() <= 255.0
            assert np.array_equal(_bits(got), _bits(_model(m, px))), m
            assert np.array_equal(_bits(got), _bits(CM.apply_np(m, px))), m
    t = fpng_amd.color_apply(TIES, every)
    assert np.array_equal(t[:, 0], ramp * np.float32(0.5))  # x.5 for every odd byte ...
    want = (ramp // 2 + ((ramp & 1) & ((ramp // 2) & 1))).astype(np.uint8)  # ... which rint takes to the even neighbour
    assert np.array_equal(CM.element_bits_np(t[:, 0], "uint8"), want) and [int(want[k]) for k in (1, 3, 5, 7)] == [0, 2, 2, 4]
    assert [CM.element_bits(float(v), "uint8") for v in t[:8, 0]] == [int(v) for v in want[:8]]
    g = fpng_amd.color_apply(CLAMP_GAIN, every)
    assert (g[:76, 0] == 0).all() and g[76, 0] == 4.0 and g[138, 0] == 252.0 and (g[139:, 0] == 255).all()
    assert np.array_equal(_bits(g[:76, 0]), np.zeros(76, dtype=np.uint32))  # (+0.0, never -0.0)
    neg = np.array([[-1, 0, 0, -0.0], [0, -0.0, 0, -0.0], [0, 0, -1, 255]], dtype=np.float32)  # (t = -0.0 for a zero byte)
    assert np.array_equal(_bits(fpng_amd.color_apply(neg, np.zeros((1, 3), dtype=np.uint8))), _bits(np.array([[0.0, 0.0, 255.0]])))


def test_the_models_two_texts_agree_where_float64_then_round_would_not():
    """fma32_np (exact product, TwoSum, round to odd, one conversion) against fma32 (integers): random values, and sums that lie
    within a float64 rounding of a binary32 tie -- where evaluating in float64 and rounding afterwards gives the wrong neighbour"""
    rng = np.random.default_rng(21)
    a = rng.uniform(-300, 300, 4000).astype(np.float32)
    b = rng.integers(0, 256, 4000).astype(np.float32)
    c = rng.uniform(-70000, 70000, 4000).astype(np.float32)
    got = CM.fma32_np(a, b, c)
    assert np.array_equal(_bits(got), _bits(np.array([CM.fma32(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], dtype=np.float32)))
    # c + 2^-24 is a tie of binary32 between c = 1 + 2^-23 and 1 + 2^-22 (the even one); the product is 2^-24 - 2^-60, so the exact
    # sum lies BELOW the tie and rounds to c, while its float64 sum is the tie itself and would round up
    x, y, z = np.float32(2.0 ** -24 * (1.0 + 2.0 ** -18)), np.float32(1.0 - 2.0 ** -18), np.float32(1.0 + 2.0 ** -23)
    assert float(x) * float(y) == 2.0 ** -24 - 2.0 ** -60
    naive = np.float32(np.float64(x) * np.float64(y) + np.float64(z))
    assert naive == np.float32(1.0 + 2.0 ** -22)  # (what "float64, then round" gives: wrong)
    assert CM.fma32(float(x), float(y), float(z)) == float(z) and CM.fma32_np(x, y, z) == z
    assert CM.fma32_np(-x, y, -z) == -z and CM.fma32(-float(x), float(y), -float(z)) == -float(z)
    # the narrow types: every binary16 / bfloat16 tie neighbourhood of a few exponents, against the integer text
    vals = np.array([v * 2.0 ** e for e in (-26, -15, -3, 0, 7) for v in (1.0, 1.0 + 2.0 ** -11, 1.0 + 2.0 ** -10, 1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -9,
                                                                        1.0 + 3 * 2.0 ** -9, 1.0 + 2.0 ** -11 + 2.0 ** -23, 1.0 + 2.0 ** -9 - 2.0 ** -23)], dtype=np.float32)
    for dtype in ("float32", "float16", "bfloat16"):
        got = CM.element_bits_np(vals, dtype, 1.0, 0.0)
        assert [int(v) for v in got] == [CM.element_bits(float(v), dtype, 1.0, 0.0) for v in vals], dtype
    assert CM.element_bits(1.0 + 2.0 ** -11, "float16") == 0x3C00 and CM.element_bits(1.0 + 3 * 2.0 ** -11, "float16") == 0x3C02  # ties to even
    assert CM.element_bits(1.0 + 2.0 ** -8, "bfloat16") == 0x3F80 and CM.element_bits(1.0 + 3 * 2.0 ** -8, "bfloat16") == 0x3F82


def _arrays(records, counts, hwc, chans=3):
    """(files, view_count, crops, views, dests, colors, results): empty destination fields in `files`, identity matrices"""
    total, n = len(records), len(counts)
    files, cnt = (_lib.PngPlanarIn * n)(), (C.c_uint32 * n)(*counts)
    c, v, d = (_lib.Crop * total)(), (_lib.ResizeView * total)(), ((_lib.ViewDestHwc if hwc else _lib.ViewDest) * total)()
    col = (_lib.ViewColor * total)()
    for k, (crop, view) in enumerate(records):
        c[k].x, c[k].y, c[k].w, c[k].h = crop
        v[k].full_w, v[k].full_h, v[k].x, v[k].y, v[k].w, v[k].h, v[k].flags, v[k].filter = view
        for ch in range(3):
            col[k].m[ch][ch] = 1.0
    for f in files:
        f.num_chans = chans
    return files, cnt, c, v, d, col, (_lib.DecodeResult * n)()


@pytest.mark.parametrize("name", PLANAR + HWC)
def test_call_level_refusals_need_no_encoder(built_lib, name):
    """with a NULL encoder every call returns -1 and the message names the reason: a bad argument its own, a good set only the
    missing encoder"""
    lib = _lib.load()
    fn, hwc = getattr(lib, name), name in HWC
    fmt = _lib.FloatFormat()

    def why():
        return lib.fpng_amd_last_error().decode()

    def fresh():
        return _arrays([GOOD[0], GOOD[1], GOOD[2]], [2, 1], hwc)

    files, cnt, c, v, d, col, res = fresh()
    good = [files, 2, cnt, c, v, d, col, None, res]
    assert fn(None, *good) == -1 and "null/empty batch" in why(), why()  # (nothing is at fault -- the batch has no encoder)
    assert fn(None, files, 2, cnt, c, v, d, col, C.byref(fmt), res) == -1 and "null/empty batch" in why(), why()
    # ---- the matrices ----
    assert fn(None, files, 2, cnt, c, v, d, None, None, res) == -1 and "null colors" in why(), why()
    for at in range(3):  # the first, a middle and the last view of the call
        for value in (float("nan"), float("inf"), float("-inf"), 65536.5, -65537.0, 3.0e38):
            for ch, k in ((0, 0), (1, 3), (2, 2)):
                files, cnt, c, v, d, col, res = fresh()
                col[at].m[ch][k] = value
                assert fn(None, files, 2, cnt, c, v, d, col, None, res) == -1 and "finite" in why() and "65536" in why(), (at, value, why())
        for value in (65536.0, -65536.0, -0.0, 1.0e-40):  # (the largest entries, a negative zero and a subnormal are fine)
            files, cnt, c, v, d, col, res = fresh()
            col[at].m[1][3] = value
            assert fn(None, files, 2, cnt, c, v, d, col, None, res) == -1 and "null/empty batch" in why(), (at, value, why())
        for flags in (1, 2, 0x80000000):
            files, cnt, c, v, d, col, res = fresh()
            col[at].flags = flags
            assert fn(None, files, 2, cnt, c, v, d, col, None, res) == -1 and "flags" in why(), (at, flags, why())
        for word in range(3):
            files, cnt, c, v, d, col, res = fresh()
            col[at].reserved[word] = 7
            assert fn(None, files, 2, cnt, c, v, d, col, None, res) == -1 and "reserved" in why(), (at, word, why())
    # ---- everything the underlying views call refuses ----
    files, cnt, c, v, d, col, res = fresh()
    good = [files, 2, cnt, c, v, d, col, None, res]
    for k in (0, 2, 3, 4, 5, 8):  # a null array
        args = list(good)
        args[k] = None
        assert fn(None, *args) == -1 and "null files, view_count, crops, views, dests or results" in why(), (k, why())
    for counts in ([0, 3], [3, 0], [0, 0]):
        assert fn(None, files, 2, (C.c_uint32 * 2)(*counts), c, v, d, col, None, res) == -1 and "view_count of 0" in why(), (counts, why())
    assert fn(None, files, 2, (C.c_uint32 * 2)(0xFFFFFFFF, 1), c, v, d, col, None, res) == -1 and "32 bits" in why(), why()
    for crop, view, word in BAD:  # every record the view call refuses, as the first, a middle and the last view of the call
        for at in range(3):
            records = [GOOD[0], GOOD[1], GOOD[2]]
            records[at] = (crop, view)
            files, cnt, c, v, d, col, res = _arrays(records, [2, 1], hwc)
            assert fn(None, files, 2, cnt, c, v, d, col, None, res) == -1 and word in why(), (crop, view, at, why())
    for field, value in (("d_pixels", 4096), ("row_pitch", -8), ("plane_pitch", 64), ("pixels_cap", 1)):
        files, cnt, c, v, d, col, res = fresh()
        setattr(files[1], field, value)
        assert fn(None, files, 2, cnt, c, v, d, col, None, res) == -1 and "must be NULL / 0" in why(), (field, why())
    if hwc:
        files, cnt, c, v, d, col, res = fresh()
        d[1].pixel_elems = 5
        assert fn(None, files, 2, cnt, c, v, d, col, None, res) == -1 and "pixel_elems" in why(), why()
        files, cnt, c, v, d, col, res = fresh()
        d[2].flags = 2
        assert fn(None, files, 2, cnt, c, v, d, col, None, res) == -1 and "fpng_amd_view_dest_hwc::flags" in why(), why()
    # ---- and a good record set of every kind fails only on the missing encoder ----
    for crop, view in GOOD:
        files, cnt, c, v, d, col, res = _arrays([(crop, view)], [1], hwc, chans=4)
        col[0].m[2][3] = -300.0
        assert fn(None, files, 1, cnt, c, v, d, col, None, res) == -1 and "null/empty batch" in why(), (crop, view, why())


def test_color_matrix():
    m = fpng_amd.color_matrix()
    assert m.dtype == np.float32 and m.shape == (3, 4) and np.array_equal(_bits(m), _bits(IDENTITY))  # exactly, and no -0.0
    luma = np.array([0.2989, 0.587, 0.114], dtype=np.float64)
    g = fpng_amd.color_matrix(saturation=0.0)
    assert np.array_equal(g[0], g[1]) and np.array_equal(g[1], g[2])
    assert np.array_equal(g[0], np.append(luma, 0.0).astype(np.float32))  # RandomGrayscale's output: the luma in all three
    # a gray pixel has no chroma: saturation and hue leave it alone, to rounding
    gray = np.array([[v, v, v, 1.0] for v in (0.0, 1.0, 100.0, 255.0)])
    for kw in ({"saturation": 0.0}, {"saturation": 0.3}, {"saturation": 1.8}, {"hue": 0.1}, {"hue": -0.5}, {"hue": 0.37, "saturation": 1.4}):
        out = gray @ fpng_amd.color_matrix(**kw).astype(np.float64).T
        # (torchvision's luma weights sum to 0.9999, so saturation s moves gray v by v * |1 - s| * 1e-4; the float32 entries' own
        #  rounding moves it by less than 255 * 4 * 2^-24 < 1e-4)
        assert np.abs(out - gray[:, :3]).max() <= 255.0 * 1e-4 * abs(1.0 - kw.get("saturation", 1.0)) + 1e-4, (kw, out)
    assert np.abs(fpng_amd.color_matrix(hue=1.0) - IDENTITY).max() < 1e-6
    assert np.abs(fpng_amd.color_matrix(hue=-1.0) - IDENTITY).max() < 1e-6
    assert np.abs(fpng_amd.color_matrix(hue=0.25) @ np.append(np.eye(3), np.zeros((1, 3)), axis=0) - np.eye(3)).max() > 0.3  # (a quarter turn is no identity)
    # positive hue moves red towards yellow and green, as torchvision's
    red = fpng_amd.color_matrix(hue=1.0 / 6.0).astype(np.float64) @ np.array([255.0, 0.0, 0.0, 1.0])
    assert red[1] > red[2] + 50 and red[0] > red[2] + 50, red
    # brightness and contrast on bytes
    x = np.arange(256, dtype=np.float64)
    for b in (0.0, 0.6, 1.0, 1.4):
        m = fpng_amd.color_matrix(brightness=b)
        assert np.array_equal(m, (IDENTITY * np.float32(b)) + np.float32(0.0))
        u = fpng_amd.color_apply(m, np.stack([x, x, x], axis=1).astype(np.uint8))
        assert np.abs(u[:, 1] - np.clip(b * x, 0, 255)).max() <= 255 * 2.0 ** -23
    for k, center in ((0.5, 128.0), (1.5, 128.0), (0.8, 117.3), (0.0, 100.0)):
        m = fpng_amd.color_matrix(contrast=k, contrast_center=center).astype(np.float64)
        assert np.allclose(m[:, :3], np.eye(3) * k, atol=1e-7) and np.allclose(m[:, 3], (1.0 - k) * center, rtol=1e-6)
        u = fpng_amd.color_apply(m, np.stack([x, x, x], axis=1).astype(np.uint8))
        assert np.abs(u[:, 2] - np.clip(k * (x - center) + center, 0, 255)).max() <= 1e-4
    # the order: brightness, then contrast, then saturation, then hue
    px = np.array([200.0, 50.0, 120.0, 1.0])
    m = fpng_amd.color_matrix(brightness=1.2, contrast=0.7, saturation=1.3, hue=0.05).astype(np.float64)
    step = px[:3] * 1.2
    step = 0.7 * (step - 128.0) + 128.0
    step = 1.3 * step + (1.0 - 1.3) * float(luma @ step)
    step = fpng_amd.color_matrix(hue=0.05).astype(np.float64) @ np.append(step, 1.0)
    assert np.abs(m @ px - step).max() < 1e-3


def test_the_color_keyword_of_the_python_door(built_lib):
    pngs = [b"\x89PNG" + bytes(60)] * 2
    crops = [[(0, 0, 90, 110)], [(0, 0, 90, 110), (1, 1, 90, 110)]]
    planar = [[torch.zeros(3, 11, 9, dtype=torch.uint8)], [torch.zeros(3, 11, 9, dtype=torch.uint8) for _ in range(2)]]
    hwc = [[torch.zeros(11, 9, 3, dtype=torch.float16)], [torch.zeros(11, 9, 3, dtype=torch.float16) for _ in range(2)]]
    a, b, c = fpng_amd.color_matrix(brightness=1.2), fpng_amd.color_matrix(saturation=0.0), fpng_amd.color_matrix(hue=0.1, contrast=0.5)
    for make, outs, cls in ((Encoder.make_decode_batch_views, planar, fpng_amd.DecodeBatchMultiView), (Encoder.make_decode_batch_views_hwc, hwc, fpng_amd.DecodeBatchMultiViewHwc)):
        assert make(pngs, crops, outs, (9, 11)).colors is None  # (None: today's call)
        assert make(pngs, crops, outs, (9, 11), color=None).colors is None
        db = make(pngs, crops, outs, (9, 11), color=a)  # one matrix for all views
        assert isinstance(db, cls) and len(db.colors) == 3 and C.sizeof(db.colors) == 192
        for rec in db.colors:
            assert np.array_equal(np.array([list(row) for row in rec.m], dtype=np.float32), a) and rec.flags == 0 and list(rec.reserved) == [0, 0, 0]
        db = make(pngs, crops, outs, (9, 11), color=a.tolist())  # (any array-like, converted to float32)
        assert np.array_equal(np.array([list(row) for row in db.colors[2].m], dtype=np.float32), a)
        db = make(pngs, crops, outs, (9, 11), color=[[a], [b, c.astype(np.float64)]])  # a list per file of a matrix per view
        for rec, m in zip(db.colors, (a, b, c)):
            assert np.array_equal(np.array([list(row) for row in rec.m], dtype=np.float32), m)
        for bad in (np.zeros((3, 3)), np.zeros((4, 4)), np.zeros(12), 1.0, "rgb", [[a], [b]], [[a, b], [c]], [[a], [b, c], [a]], [a, b, c], [[a], [b, np.zeros((3, 3))]],
                    [[a], b], np.zeros((3, 3, 4))):
            with pytest.raises(ValueError):
                make(pngs, crops, outs, (9, 11), color=bad)
    with pytest.raises(ValueError):
        fpng_amd.color_apply(np.zeros((3, 3)), np.zeros((1, 3), dtype=np.uint8))
    with pytest.raises(ValueError):
        fpng_amd.color_apply(IDENTITY, np.zeros((5, 4), dtype=np.uint8))
    assert fpng_amd.color_apply(IDENTITY, np.zeros((2, 5, 3), dtype=np.uint8)).shape == (2, 5, 3)
