"""No-GPU tests of the per-view tone record of the views calls (fpng_amd_decode_batch(_device)_planar_views_tone / _hwc_views_tone):
the exact model of tone_model.py and the host twins fpng_amd_view_tone_lut / fpng_amd_view_tone_apply -- the text the kernel runs --
against Pillow's ImageOps.autocontrast, ImageOps.equalize and ImageEnhance.Contrast, whole images bit for bit; the table twin
exhaustively where that is cheap; every call-level refusal, none of which needs an encoder or a device; the Python door; the twins
under the sanitizers."""
import ctypes as C
import math

import numpy as np
import pytest
import torch
from PIL import Image, ImageEnhance, ImageOps

import fpng_amd
from fpng_amd import _lib
from fpng_amd.api import Encoder

import tone_model as TM
from test_resize_view_cpu import GOOD
from test_views_post_cpu import _arrays, _fill as _fill_post
from test_views_warp_cpu import _fill as _fill_warp

PLANAR = ("fpng_amd_decode_batch_planar_views_tone", "fpng_amd_decode_batch_device_planar_views_tone")
HWC = ("fpng_amd_decode_batch_hwc_views_tone", "fpng_amd_decode_batch_device_hwc_views_tone")
KINDS = ("random", "narrow", "three", "gaussian", "solid")
AUTO, EQUAL, CONTRAST = _lib.TONE_AUTOCONTRAST, _lib.TONE_EQUALIZE, _lib.TONE_CONTRAST


def _image(kind, w, h, rng):
    """(h, w, 3) bytes of one of the five kinds"""
    if kind == "random":
        a = rng.integers(0, 256, size=(h, w, 3))
    elif kind == "narrow":
        lo = rng.integers(0, 250, size=3)
        a = lo + rng.integers(0, int(rng.integers(2, 40)), size=(h, w, 3))
    elif kind == "three":
        a = rng.choice(rng.integers(0, 256, size=3), size=(h, w, 3))
    elif kind == "gaussian":
        a = rng.normal(rng.uniform(40, 215), rng.uniform(3, 60), size=(h, w, 3))
    else:
        a = np.broadcast_to(rng.integers(0, 256, size=3), (h, w, 3))
    return np.ascontiguousarray(np.clip(np.rint(a), 0, 255).astype(np.uint8))


def _record(tone):
    return fpng_amd.view_tone(**tone)


def _pillow(tone, img):
    pil = Image.fromarray(img)
    if tone.get("autocontrast"):
        return np.asarray(ImageOps.autocontrast(pil))
    if tone.get("equalize"):
        return np.asarray(ImageOps.equalize(pil))
    return np.asarray(ImageEnhance.Contrast(pil).enhance(float(np.float32(tone["contrast"]))))


def _all_three(tone, img):
    """(model, apply twin, table twin on the model's histograms) for the (h, w, 3) image"""
    planes = np.ascontiguousarray(img.transpose(2, 0, 1))
    lut = fpng_amd.view_tone_lut(_record(tone), TM.histograms(planes))
    return (TM.apply(tone, planes).transpose(1, 2, 0), fpng_amd.view_tone_apply(_record(tone), planes).transpose(1, 2, 0),
            np.stack([lut[c][planes[c]] for c in range(3)], axis=-1))


def _clamped_equalize_image():
    """one channel of 0 x 1, 1 x 1000, 2 x 75753, 255 x 6 -- 76760 = 380 x 202 samples: step 300 and an unclamped lut[255] of 256"""
    ch = np.concatenate([np.full(1, 0), np.full(1000, 1), np.full(75753, 2), np.full(6, 255)]).astype(np.uint8)
    assert ch.size == 380 * 202
    rng = np.random.default_rng(5)
    return np.ascontiguousarray(np.stack([rng.permutation(ch).reshape(202, 380) for _ in range(3)], axis=-1))


def test_entry_points_and_record(built_lib):
    lib = _lib.load()
    for name in PLANAR + HWC + ("fpng_amd_view_tone_lut", "fpng_amd_view_tone_apply"):
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
    assert lib.fpng_amd_abi_version() == 5  # (new entry points, the same ABI version)
    assert C.sizeof(_lib.ViewTone) == 16
    assert {n: getattr(_lib.ViewTone, n).offset for n, _ in _lib.ViewTone._fields_} == {"op": 0, "factor": 4, "reserved": 8}
    assert (AUTO, EQUAL, CONTRAST) == (1, 2, 3)


# ---- against Pillow ----
def test_the_model_and_the_host_twins_are_pillows(built_lib):
    """the five kinds of image, every width and every height 1 .. 40 (each width with three heights), all three operations; contrast
    with 0 or 1, one factor in [0, 1], one in (1, 2] and one up to 100 per image: the model, the apply twin and the table twin all
    give Pillow's whole image"""
    rng = np.random.default_rng(20240611)
    n, seen_h = 0, set()
    for w in range(1, 41):
        for k in range(3):
            h = (w * 3 + k * 13) % 40 + 1
            seen_h.add(h)
            for kind in KINDS:
                img = _image(kind, w, h, rng)
                factors = [float(n & 1), rng.uniform(0, 1), rng.uniform(1, 2), rng.uniform(2, 100)]
                for tone in [{"autocontrast": True}, {"equalize": True}] + [{"contrast": float(np.float32(f))} for f in factors]:
                    want = _pillow(tone, img)
                    for name, got in zip(("model", "apply twin", "table twin"), _all_three(tone, img)):
                        assert np.array_equal(got, want), (name, kind, w, h, tone, int(np.count_nonzero(got != want)))
                n += 1
    assert n == 600 and seen_h == set(range(1, 41))


def test_contrast_factors_up_to_100_are_pillows(built_lib):
    """the clamped branch on a sweep of factors: every quarter up to 4, then every 1.75 up to 100, and fp32 neighbours of 1"""
    rng = np.random.default_rng(3)
    img = _image("random", 23, 17, rng)
    dark = _image("gaussian", 9, 31, rng)
    factors = [k * 0.25 for k in range(17)] + [4 + k * 1.75 for k in range(55)] + [float(np.nextafter(np.float32(1), np.float32(2))), float(np.nextafter(np.float32(1), np.float32(0)))]
    assert max(factors) > 98
    for f in factors:
        for im in (img, dark):
            want = _pillow({"contrast": f}, im)
            for name, got in zip(("model", "apply twin", "table twin"), _all_three({"contrast": f}, im)):
                assert np.array_equal(got, want), (name, f, int(np.count_nonzero(got != want)))


def test_equalize_clips_its_table_as_pillow_does(built_lib):
    img = _clamped_equalize_image()
    h = TM.histograms(img.transpose(2, 0, 1))
    entries = TM.equalize_entries(h[0])
    assert (sum(int(x) for x in h[0]) - int(h[0][255])) // 255 == 300 and entries[255] == 256  # (the min of the rule is real)
    want = _pillow({"equalize": True}, img)
    for name, got in zip(("model", "apply twin", "table twin"), _all_three({"equalize": True}, img)):
        assert np.array_equal(got, want), (name, int(np.count_nonzero(got != want)))
    assert want.max() == 255


# ---- fpng_amd_view_tone_lut, exhaustively where that is cheap ----
def _hist(**bins):
    h = np.zeros((4, 256), dtype=np.int64)
    for c, counts in bins.items():
        for v, x in counts.items():
            h[int(c[1:]), v] = x
    return h


def test_autocontrast_tables_for_every_lo_and_hi(built_lib):
    """all 32 640 pairs lo < hi (the three channels carry three pairs at once), against Python's own double arithmetic"""
    rec = fpng_amd.view_tone(autocontrast=True)
    pairs = [(lo, hi) for lo in range(256) for hi in range(lo + 1, 256)]
    assert len(pairs) == 32640
    for k in range(0, len(pairs), 3):
        h = np.zeros((4, 256), dtype=np.int64)
        for c, (lo, hi) in enumerate(pairs[k:k + 3]):
            h[c, lo], h[c, hi] = 1 + (lo & 3), 7
            h[c, (lo + hi) // 2] += 2
        lut = fpng_amd.view_tone_lut(rec, h)
        for c, (lo, hi) in enumerate(pairs[k:k + 3]):
            scale = 255.0 / (hi - lo)
            offset = -lo * scale
            want = [min(max(int(v * scale + offset), 0), 255) for v in range(256)]
            assert lut[c].tolist() == want, (lo, hi)
            assert lut[c][lo] == 0 and lut[c][hi] in (254, 255)
    # (one bin, and none: the identity)
    ident = list(range(256))
    assert fpng_amd.view_tone_lut(rec, _hist(c0={9: 5}, c1={255: 1}, c2={0: 0xFFFFFFFF}))[:].tolist() == [ident] * 3
    assert fpng_amd.view_tone_lut(rec, np.zeros((4, 256), dtype=np.int64)).tolist() == [ident] * 3


def test_contrast_tables_for_every_mean(built_lib):
    """every mean 0 .. 255 (a one-bin luma histogram) with a grid of factors, against the fp32 formula in numpy; means that round"""
    factors = [0.0, 1.0, 0.5, 0.1, 0.9, 1.0 / 3, 0.999999, 1.0000001, 1.5, 1.9, 2.0, 3.7, 10.0, 64.5, 100.0, 1e-30, 3.0e38]
    for mean in range(256):
        h = np.zeros((4, 256), dtype=np.int64)
        h[3, mean] = 1 + mean
        for f in factors:
            lut = fpng_amd.view_tone_lut(fpng_amd.view_tone(contrast=f), h)
            want = TM.contrast_lut_of_mean(mean, np.float32(f))
            assert np.array_equal(lut, np.stack([want] * 3)), (mean, f)
            if f <= 1.0:
                assert lut[0][mean] == mean
    # the mean is int(sum / count + 0.5): exact halves go up, and nothing else does; counts near 2^32
    for bins, mean in (({10: 1, 11: 1}, 11), ({10: 2, 11: 1}, 10), ({10: 1, 11: 2}, 11), ({0: 0xFFFFFFFF}, 0), ({255: 0xFFFFFFFF}, 255), ({254: 0x7FFFFFFF, 255: 0x80000000}, 255),
                       ({254: 0x80000000, 255: 0x7FFFFFFF}, 254), ({0: 3, 255: 1}, 64), ({0: 1, 255: 3}, 191)):
        h = _hist(c3=bins)
        assert TM.contrast_mean(h[3]) == mean
        assert np.array_equal(fpng_amd.view_tone_lut(fpng_amd.view_tone(contrast=0.0), h), np.full((3, 256), mean, dtype=np.uint8)), bins


def test_equalize_tables_for_synthetic_histograms(built_lib):
    """step 0, 1 and large, one non-zero bin, counts near 2^32 (sums past it: the rule's integers are 64 bits wide), the clamp"""
    rec = fpng_amd.view_tone(equalize=True)
    big = 0xFFFFFFFF
    rng = np.random.default_rng(8)
    cases = [{5: 100}, {5: 254, 200: big}, {5: 255, 200: 1}, {0: 1, 255: 1}, {3: 254, 4: 1, 9: 7}, {3: 255, 9: 7}, {0: 1, 1: 1000, 2: 75753, 255: 6},
             {v: big for v in range(256)}, {v: big for v in range(0, 256, 5)}, {0: big, 255: 1}, {0: 1, 255: big}, {17: big - 1, 18: big, 19: 3},
             {v: 1 for v in range(256)}, {v: 2 for v in range(256)}, {v: v + 1 for v in range(256)}]
    cases += [{int(v): int(rng.integers(1, 2 ** 32)) for v in rng.choice(256, size=int(rng.integers(2, 40)), replace=False)} for _ in range(30)]
    steps = set()
    for k in range(0, len(cases), 3):
        three = (cases[k:k + 3] * 3)[:3]
        h = _hist(c0=three[0], c1=three[1], c2=three[2])
        lut = fpng_amd.view_tone_lut(rec, h)
        for c in range(3):
            assert np.array_equal(lut[c], TM.equalize_lut(h[c])), three[c]
            nz = [int(x) for x in h[c] if x]
            steps.add(min((sum(nz) - nz[-1]) // 255, 2) if len(nz) > 1 else -1)
    assert steps == {-1, 0, 1, 2}
    assert np.array_equal(fpng_amd.view_tone_lut(rec, _hist(c0={0: 1, 1: 1000, 2: 75753, 255: 6}))[0][[0, 1, 2, 3, 255]], [0, 0, 3, 255, 255])
    # (a record without an op: the identity, whatever the histograms)
    assert fpng_amd.view_tone_lut(fpng_amd.view_tone(), _hist(c0={1: 9, 7: 9}, c3={4: 2})).tolist() == [list(range(256))] * 3


# ---- refusals ----
NAN, INF = float("nan"), float("inf")
# (op, factor, reserved) and a piece of the message; the record's view is GOOD[1]: a 6 x 4 window
BAD_RECORDS = [((4, 0.0, (0, 0)), "unknown fpng_amd_view_tone::op"), ((0xFFFFFFFF, 0.0, (0, 0)), "unknown fpng_amd_view_tone::op"), ((0x80000001, 0.0, (0, 0)), "unknown fpng_amd_view_tone::op"),
               ((AUTO, 0.0, (1, 0)), "fpng_amd_view_tone::reserved must be 0"), ((0, 0.0, (0, 5)), "fpng_amd_view_tone::reserved must be 0"),
               ((CONTRAST, NAN, (0, 0)), "finite and >= 0 with FPNG_AMD_TONE_CONTRAST"), ((CONTRAST, INF, (0, 0)), "finite and >= 0 with FPNG_AMD_TONE_CONTRAST"),
               ((CONTRAST, -INF, (0, 0)), "finite and >= 0 with FPNG_AMD_TONE_CONTRAST"), ((CONTRAST, -1e-40, (0, 0)), "finite and >= 0 with FPNG_AMD_TONE_CONTRAST"),
               ((CONTRAST, -1.0, (0, 0)), "finite and >= 0 with FPNG_AMD_TONE_CONTRAST"),
               ((0, 1.0, (0, 0)), "must be 0 without FPNG_AMD_TONE_CONTRAST"), ((AUTO, 1e-40, (0, 0)), "must be 0 without FPNG_AMD_TONE_CONTRAST"),
               ((EQUAL, NAN, (0, 0)), "must be 0 without FPNG_AMD_TONE_CONTRAST"), ((EQUAL, -2.0, (0, 0)), "must be 0 without FPNG_AMD_TONE_CONTRAST")]
GOOD_RECORDS = [(0, 0.0, (0, 0)), (0, -0.0, (0, 0)), (AUTO, 0.0, (0, 0)), (EQUAL, -0.0, (0, 0)), (CONTRAST, 0.0, (0, 0)), (CONTRAST, -0.0, (0, 0)), (CONTRAST, 1.0, (0, 0)),
                (CONTRAST, 3.0e38, (0, 0)), (CONTRAST, 1e-45, (0, 0))]
# a window of 65537 x 65536 samples: one more row than uint32 counts
HUGE = ((0, 0, 96, 64), (65537, 65536, 0, 0, 65537, 65536, 0, 0))
EDGE = ((0, 0, 96, 64), (65537, 65536, 0, 0, 65535, 65537, 0, 0))  # (65535 * 65537 = 2^32 - 1: it fits)


def _fill(rec, values):
    rec.op, rec.factor = values[0], values[1]
    rec.reserved[0], rec.reserved[1] = values[2]


@pytest.mark.parametrize("name", PLANAR + HWC)
def test_call_level_refusals_need_no_encoder(built_lib, name):
    """with a NULL encoder every call returns -1 and the message names the reason: a bad argument its own, a good set only the
    missing encoder"""
    lib = _lib.load()
    fn, hwc = getattr(lib, name), name in HWC
    fmt = _lib.FloatFormat()

    def why():
        return lib.fpng_amd_last_error().decode()

    def fresh(records=(GOOD[0], GOOD[1], GOOD[2])):  # the second record's window is 6 x 4
        files, cnt, c, v, d, col, post, res = _arrays(list(records), [2, 1], hwc)
        return files, cnt, c, v, d, col, post, (_lib.ViewWarp * 3)(), (_lib.ViewTone * 3)(), res

    files, cnt, c, v, d, col, post, warp, tone, res = fresh()
    for colors in (col, None):  # (NULL colors, posts and warps: the identity, no flags, no warp)
        for posts in (post, None):
            for warps in (warp, None):
                assert fn(None, files, 2, cnt, c, v, d, colors, posts, warps, tone, None, res) == -1 and "null/empty batch" in why(), why()  # (nothing is at fault but the missing encoder)
                assert fn(None, files, 2, cnt, c, v, d, colors, posts, warps, tone, C.byref(fmt), res) == -1 and "null/empty batch" in why(), why()
                assert fn(None, files, 2, cnt, c, v, d, colors, posts, warps, None, None, res) == -1 and "null tones" in why(), why()
    # ---- the records ----
    for others in (True, False):
        for values, piece in BAD_RECORDS:
            files, cnt, c, v, d, col, post, warp, tone, res = fresh()
            _fill(tone[1], values)
            assert fn(None, files, 2, cnt, c, v, d, col, post if others else None, warp if others else None, tone, None, res) == -1 and piece in why(), (values, why())
        for values in GOOD_RECORDS:
            files, cnt, c, v, d, col, post, warp, tone, res = fresh()
            _fill(tone[2], values)  # (the last record of the call is judged too)
            assert fn(None, files, 2, cnt, c, v, d, col, post if others else None, warp if others else None, tone, None, res) == -1 and "null/empty batch" in why(), (values, why())
    files, cnt, c, v, d, col, post, warp, tone, res = fresh()
    _fill(tone[2], BAD_RECORDS[0][0])
    assert fn(None, files, 2, cnt, c, v, d, col, post, warp, tone, None, res) == -1 and "fpng_amd_view_tone::op" in why(), why()
    # ---- w * h beyond uint32: refused for a view with an op, of no concern to one without ----
    for at in (0, 1, 2):
        for op in (AUTO, EQUAL, CONTRAST):
            files, cnt, c, v, d, col, post, warp, tone, res = fresh([HUGE if k == at else GOOD[k] for k in range(3)])
            tone[at].op = op
            assert fn(None, files, 2, cnt, c, v, d, col, post, warp, tone, None, res) == -1 and "w * h must fit 32 bits" in why(), (at, op, why())
            tone[at].op, tone[(at + 1) % 3].op = 0, op
            assert fn(None, files, 2, cnt, c, v, d, col, post, warp, tone, None, res) == -1 and "w * h must fit 32 bits" not in why(), (at, op, why())
        files, cnt, c, v, d, col, post, warp, tone, res = fresh([EDGE if k == at else GOOD[k] for k in range(3)])
        tone[at].op = EQUAL
        assert fn(None, files, 2, cnt, c, v, d, col, post, warp, tone, None, res) == -1 and "w * h must fit 32 bits" not in why(), (at, why())
    # ---- everything the warp call refuses ----
    files, cnt, c, v, d, col, post, warp, tone, res = fresh()
    _fill(tone[0], GOOD_RECORDS[2])
    _fill_warp(warp[1], (4, 0, (1.0, 0.0, 0.0, 0.0, 1.0, 0.0), (0, 0, 0, 0), 0))
    assert fn(None, files, 2, cnt, c, v, d, col, post, warp, tone, None, res) == -1 and "unknown fpng_amd_view_warp::flags" in why(), why()
    _fill_warp(warp[1], (1, 0, (1.0, 0.0, 32768.0, 0.0, 1.0, 0.0), (0, 0, 0, 0), 0))
    assert fn(None, files, 2, cnt, c, v, d, col, post, warp, tone, None, res) == -1 and "check_fixed" in why(), why()
    _fill_warp(warp[1], (1, 0, (1.0, 0.1, 0.0, 0.0, 1.0, 0.0), (1, 2, 3, 4), 0))
    _fill_post(post[1], (_lib.POST_BLUR, 4, 1.0, 0, 0, (0, 0)))
    assert fn(None, files, 2, cnt, c, v, d, col, post, warp, tone, None, res) == -1 and "below the window" in why(), why()
    _fill_post(post[1], (_lib.POST_SOLARIZE, 0, 0.0, 256, 0, (0, 0)))
    assert fn(None, files, 2, cnt, c, v, d, col, post, warp, tone, None, res) == -1 and "solarize_threshold" in why(), why()
    _fill_post(post[1], (_lib.POST_BLUR, 3, 1.0, 0, 0, (0, 0)))
    col[2].m[1][1] = float("nan")
    assert fn(None, files, 2, cnt, c, v, d, col, post, warp, tone, None, res) == -1 and "fpng_amd_view_color::m" in why(), why()
    col[2].m[1][1] = 1.0
    good = [files, 2, cnt, c, v, d, col, post, warp, tone, None, res]
    assert fn(None, *good) == -1 and "null/empty batch" in why(), why()
    for k in (0, 2, 3, 4, 5, 11):  # a null array
        args = list(good)
        args[k] = None
        assert fn(None, *args) == -1 and "null files, view_count, crops, views, dests or results" in why(), (k, why())
    for counts in ([0, 3], [3, 0]):
        assert fn(None, files, 2, (C.c_uint32 * 2)(*counts), c, v, d, col, post, warp, tone, None, res) == -1 and "view_count of 0" in why(), (counts, why())
    v[1].filter = 2
    assert fn(None, *good) == -1 and "filter" in why(), why()
    v[1].filter = 1
    files[1].row_pitch = 4
    assert fn(None, *good) == -1 and "must be NULL / 0" in why(), why()


def test_the_host_twins_refuse_what_the_calls_refuse(built_lib):
    lib = _lib.load()
    planes = np.zeros((3, 4, 6), dtype=np.uint8)
    out = np.zeros_like(planes)
    hist = np.zeros((4, 256), dtype=np.uint32)
    lut = np.zeros((3, 256), dtype=np.uint8)
    for values, piece in BAD_RECORDS:
        rec = _lib.ViewTone()
        _fill(rec, values)
        for call in (lambda: fpng_amd.view_tone_apply(rec, planes), lambda: fpng_amd.view_tone_lut(rec, hist)):
            with pytest.raises(fpng_amd.FpngAmdError, match=piece.replace("(", r"\(").replace(")", r"\)")):
                call()
    for values in GOOD_RECORDS:
        rec = _lib.ViewTone()
        _fill(rec, values)
        fpng_amd.view_tone_apply(rec, planes)
        fpng_amd.view_tone_lut(rec, hist)
    rec = fpng_amd.view_tone(equalize=True)
    assert lib.fpng_amd_view_tone_apply(C.byref(rec), 65537, 65536, planes.ctypes.data, out.ctypes.data) == -1 and "w * h must fit 32 bits" in lib.fpng_amd_last_error().decode()
    assert lib.fpng_amd_view_tone_apply(None, 6, 4, planes.ctypes.data, out.ctypes.data) == -1
    assert lib.fpng_amd_view_tone_apply(C.byref(rec), 6, 4, None, out.ctypes.data) == -1
    assert lib.fpng_amd_view_tone_apply(C.byref(rec), 6, 4, planes.ctypes.data, None) == -1
    assert lib.fpng_amd_view_tone_apply(C.byref(rec), 0, 4, planes.ctypes.data, out.ctypes.data) == -1
    assert lib.fpng_amd_view_tone_apply(C.byref(rec), 6, 0, planes.ctypes.data, out.ctypes.data) == -1
    assert lib.fpng_amd_view_tone_lut(None, hist.ctypes.data, lut.ctypes.data) == -1
    assert lib.fpng_amd_view_tone_lut(C.byref(rec), None, lut.ctypes.data) == -1
    assert lib.fpng_amd_view_tone_lut(C.byref(rec), hist.ctypes.data, None) == -1


# ---- the Python door ----
def test_view_tone():
    r = fpng_amd.view_tone()
    assert (r.op, r.factor, list(r.reserved)) == (0, 0.0, [0, 0])
    assert (fpng_amd.view_tone(autocontrast=True).op, fpng_amd.view_tone(equalize=True).op) == (AUTO, EQUAL)
    r = fpng_amd.view_tone(contrast=0.1)
    assert (r.op, r.factor) == (CONTRAST, float(np.float32(0.1))) and r.factor != 0.1  # (rounded to fp32 once)
    assert (fpng_amd.view_tone(contrast=0).op, fpng_amd.view_tone(contrast=0).factor) == (CONTRAST, 0.0)  # (a factor of 0 is an operation: the solid mean)
    assert fpng_amd.view_tone(contrast=np.float32(1.5)).factor == 1.5 and fpng_amd.view_tone(autocontrast=False, equalize=False, contrast=None).op == 0
    for bad in ({"autocontrast": True, "equalize": True}, {"autocontrast": True, "contrast": 1.0}, {"equalize": True, "contrast": 0.0}, {"autocontrast": True, "equalize": True, "contrast": 2},
                {"contrast": -0.5}, {"contrast": NAN}, {"contrast": INF}, {"contrast": 1e39}, {"contrast": "much"}, {"contrast": [1.0, 2.0]}):
        with pytest.raises(ValueError):
            fpng_amd.view_tone(**bad)
    good = fpng_amd.view_tone(equalize=True)
    for bad in (lambda: fpng_amd.view_tone_apply({"equalize": True}, np.zeros((3, 2, 2), dtype=np.uint8)), lambda: fpng_amd.view_tone_apply(good, np.zeros((2, 2), dtype=np.uint8)),
                lambda: fpng_amd.view_tone_apply(good, np.full((3, 2, 2), 300, dtype=np.int64)), lambda: fpng_amd.view_tone_apply(good, np.zeros((3, 2, 2), dtype=np.float32)),
                lambda: fpng_amd.view_tone_apply(good, [[[1, 2]], [[3, 4]], [[5, 6]]]),
                lambda: fpng_amd.view_tone_apply(good, np.zeros((4, 2, 2), dtype=np.uint8)), lambda: fpng_amd.view_tone_apply(good, np.zeros((3, 0, 2), dtype=np.uint8)),
                lambda: fpng_amd.view_tone_lut({"equalize": True}, np.zeros((4, 256), dtype=np.int64)), lambda: fpng_amd.view_tone_lut(good, np.zeros((3, 256), dtype=np.int64)),
                lambda: fpng_amd.view_tone_lut(good, np.zeros((4, 256), dtype=np.float32)), lambda: fpng_amd.view_tone_lut(good, np.full((4, 256), -1, dtype=np.int64)),
                lambda: fpng_amd.view_tone_lut(good, np.full((4, 256), 2 ** 32, dtype=np.int64))):
        with pytest.raises(ValueError):
            bad()


@pytest.mark.parametrize("hwc", [False, True])
def test_the_tone_keyword_shapes_and_lengths(hwc):
    """make_decode_batch_views(_hwc)(..., tone=) needs no GPU: one record, one per file, one per view; wrong lengths and types raise"""
    make = Encoder.make_decode_batch_views_hwc if hwc else Encoder.make_decode_batch_views
    pngs = [b"x" * 8, b"y" * 8]
    crops = [[(0, 0, 8, 8), (1, 1, 4, 4)], [(0, 0, 8, 8)]]
    outs = [[torch.empty((4, 4, 3) if hwc else (3, 4, 4), dtype=torch.uint8) for _ in cs] for cs in crops]
    a, b = fpng_amd.view_tone(autocontrast=True), fpng_amd.view_tone(contrast=1.5)
    assert make(pngs, crops, outs, (4, 4)).tones is None and make(pngs, crops, outs, (4, 4), post=fpng_amd.view_post(solarize=1), warp=fpng_amd.view_warp()).tones is None
    db = make(pngs, crops, outs, (4, 4), tone=a)
    assert db.colors is None and db.posts is None and db.warps is None and [(p.op, p.factor) for p in db.tones] == [(AUTO, 0.0)] * 3
    db = make(pngs, crops, outs, (4, 4), tone=[a, b])
    assert [(p.op, p.factor) for p in db.tones] == [(AUTO, 0.0), (AUTO, 0.0), (CONTRAST, 1.5)]
    db = make(pngs, crops, outs, (4, 4), tone=[[b, a], [fpng_amd.view_tone()]], color=np.eye(3, 4), post=fpng_amd.view_post(posterize=2), warp=fpng_amd.view_warp())
    assert db.colors is not None and db.posts is not None and db.warps is not None and [p.op for p in db.tones] == [CONTRAST, AUTO, 0]
    for bad in ([a], [a, b, a], [[a], [b]], [[a, b, a], b], [[a, b], []], 3, [a, 3], [[a, {"equalize": True}], b], "ab", fpng_amd.view_post(), fpng_amd.view_warp()):
        with pytest.raises(ValueError):
            make(pngs, crops, outs, (4, 4), tone=bad)


# ---- the host twins under the sanitizers ----
def _sanitizer_planes(w, h, kind):
    x, y = np.arange(w, dtype=np.int64)[None, :], np.arange(h, dtype=np.int64)[:, None]
    if kind == 0:
        return np.stack([((7 * x + 13 * y + x * y + 50 * c) & 255) for c in range(3)]).astype(np.uint8)
    if kind == 1:
        return np.stack([np.full((h, w), 17 + c) for c in range(3)]).astype(np.uint8)
    if kind == 2:
        return np.stack([np.where((x + y) & 1, 200, 3 + c) for c in range(3)]).astype(np.uint8)
    return np.stack([100 + (x + 3 * y + c) % 7 for c in range(3)]).astype(np.uint8)


def _sanitizer_cases():
    """(w, h, kind, op, reserved, factor): every edge shape with every kind of image and every op; and records the calls refuse"""
    out = []
    sizes = [(w, h) for w in (1, 2, 3, 17, 64, 65, 130) for h in (1, 2, 16, 17, 33)] + [(380, 202)]
    for n, (w, h) in enumerate(sizes):
        for kind in range(4):
            out += [(w, h, kind, 0, 0, 0.0), (w, h, kind, AUTO, 0, 0.0), (w, h, kind, EQUAL, 0, 0.0)]
            out += [(w, h, kind, CONTRAST, 0, f) for f in (0.0, 1.0, float(np.float32(0.37 + 0.01 * n)), 1.0 + 0.25 * kind + 0.001 * n, 99.5, 3.0e38)]
    out += [(6, 4, 0, 4, 0, 0.0), (6, 4, 0, AUTO, 1, 0.0), (6, 4, 1, CONTRAST, 0, NAN), (6, 4, 2, CONTRAST, 0, -1.0), (6, 4, 3, EQUAL, 0, 2.0), (6, 4, 0, 0, 0, INF)]
    return out


def test_the_host_twins_under_the_sanitizers(built_lib, tmp_path):
    """tests/cpp/view_tone_apply.cpp, a stand-alone program over view_tone.h built with the address and undefined-behaviour
    sanitizers and run on the CPU: no report, and every table and view it prints is the model's"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "view_tone_apply")
    # (-Wno-unknown-pragmas: the header's `#pragma clang fp contract`; g++ in ISO mode does not contract on x86-64.  The sanitizers'
    #  runtimes are linked into the program where the compiler has them as archives, so that it starts in any environment)
    cmd = ["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-I", os.path.join(root, "fpng_amd", "csrc"),
           "-I", os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "view_tone_apply.cpp"), "-o", exe]
    r = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if r.returncode != 0:
        r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    cases = _sanitizer_cases()
    text = "".join("%d %d %d %d %d %s\n" % (w, h, kind, op, reserved, float(np.float32(f)).hex()) for w, h, kind, op, reserved, f in cases)
    env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([exe], input=text, capture_output=True, text=True, env=env, timeout=120)
    assert run.returncode == 0 and not run.stderr, (run.returncode, run.stderr[-2000:])
    lines = run.stdout.splitlines()
    assert len(lines) == len(cases)
    refused = 0
    for (w, h, kind, op, reserved, f), ln in zip(cases, lines):
        ok = op <= 3 and not reserved and (math.isfinite(f) and f >= 0 if op == CONTRAST else f == 0)
        if not ok:
            assert ln.startswith("refused "), (w, h, kind, op, f, ln[:80])
            refused += 1
            continue
        tone = {AUTO: {"autocontrast": True}, EQUAL: {"equalize": True}, CONTRAST: {"contrast": float(np.float32(f))}, 0: {}}[op]
        planes = _sanitizer_planes(w, h, kind)
        want = "ok " + TM.luts(tone, TM.histograms(planes)).tobytes().hex() + " " + TM.apply(tone, planes).tobytes().hex()
        assert ln == want, (w, h, kind, op, f)
    assert refused == 6
