"""No-GPU tests of the per-view enhance record of the views calls (fpng_amd_decode_batch(_device)_planar_views_enhance /
_hwc_views_enhance): the exact model of enhance_model.py and the host twin fpng_amd_view_enhance_apply -- the text the kernel runs
-- against Pillow's ImageEnhance.Brightness, ImageEnhance.Color and ImageEnhance.Sharpness, whole images bit for bit; every
call-level refusal, none of which needs an encoder or a device; the Python door; the twin under the sanitizers; rotate_matrix()
against Image.rotate and augment_op() against the Pillow call of each of its fourteen names."""
import ctypes as C
import math

import numpy as np
import pytest
import torch
from PIL import Image, ImageEnhance, ImageOps

import fpng_amd
from fpng_amd import _lib
from fpng_amd.api import Encoder

import enhance_model as EM
from test_resize_view_cpu import GOOD
from test_views_post_cpu import _arrays, _fill as _fill_post
from test_views_tone_cpu import _fill as _fill_tone
from test_views_warp_cpu import _fill as _fill_warp

PLANAR = ("fpng_amd_decode_batch_planar_views_enhance", "fpng_amd_decode_batch_device_planar_views_enhance")
HWC = ("fpng_amd_decode_batch_hwc_views_enhance", "fpng_amd_decode_batch_device_hwc_views_enhance")
BRIGHT, COLOR, SHARP = _lib.ENHANCE_BRIGHTNESS, _lib.ENHANCE_COLOR, _lib.ENHANCE_SHARPNESS
NAMES = {BRIGHT: "brightness", COLOR: "color", SHARP: "sharpness"}
PILLOW = {"brightness": ImageEnhance.Brightness, "color": ImageEnhance.Color, "sharpness": ImageEnhance.Sharpness}
NAN, INF = float("nan"), float("inf")
FACTORS = (0.0, 0.37, 1.0, 1.9, 4.0)  # 0, a value in (0, 1), 1, 1.9 and a large one
# (op, factor, reserved) and a piece of the message
BAD_RECORDS = [((4, 1.0, (0, 0)), "fpng_amd_view_enhance::op"), ((0xFFFFFFFF, 0.0, (0, 0)), "fpng_amd_view_enhance::op"),
               ((BRIGHT, 1.0, (1, 0)), "reserved"), ((0, 0.0, (0, 7)), "reserved"),
               ((BRIGHT, NAN, (0, 0)), "finite and >= 0"), ((COLOR, INF, (0, 0)), "finite and >= 0"), ((SHARP, -0.5, (0, 0)), "finite and >= 0"),
               ((SHARP, -INF, (0, 0)), "finite and >= 0"),
               ((0, 1.0, (0, 0)), "must be 0 without an op"), ((0, NAN, (0, 0)), "must be 0 without an op"), ((0, -1.0, (0, 0)), "must be 0 without an op")]
GOOD_RECORDS = [(0, 0.0, (0, 0)), (0, -0.0, (0, 0)), (BRIGHT, 0.0, (0, 0)), (COLOR, 1.0, (0, 0)), (SHARP, 3.0e38, (0, 0)), (BRIGHT, -0.0, (0, 0))]


def _images(rng):
    """(h, w, 3) uint8 images: every h and w of 1, 2, 3 against each other and against larger ones, random sizes up to 40 x 40; full-range
    noise and low-entropy images (values in {0, 85, 170, 255}), so that the blend clips at both ends"""
    sizes = [(h, w) for h in (1, 2, 3) for w in (1, 2, 3, 4, 17, 40)] + [(h, w) for w in (1, 2, 3) for h in (4, 17, 40)]
    sizes += [tuple(int(v) for v in rng.integers(4, 41, size=2)) for _ in range(60)]
    for k, (h, w) in enumerate(sizes):
        if k % 3 == 2:
            yield rng.choice(np.array([0, 85, 170, 255], dtype=np.uint8), size=(h, w, 3))
        else:
            yield rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def _fill(rec, values):
    rec.op, rec.factor = values[0], values[1]
    rec.reserved[0], rec.reserved[1] = values[2]


def test_entry_points_and_record(built_lib):
    lib = _lib.load()
    for name in PLANAR + HWC + ("fpng_amd_view_enhance_apply",):
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
    assert lib.fpng_amd_abi_version() == 5  # (new entry points, the same ABI version)
    assert C.sizeof(_lib.ViewEnhance) == 16
    assert {n: getattr(_lib.ViewEnhance, n).offset for n, _ in _lib.ViewEnhance._fields_} == {"op": 0, "factor": 4, "reserved": 8}
    assert (BRIGHT, COLOR, SHARP) == (1, 2, 3)


# ---- against Pillow ----
def test_the_model_and_the_host_twin_are_pillows(built_lib):
    """the images of _images under the three operations at the five factors: the model and the twin both give Pillow's whole image,
    and clipping at both ends occurs"""
    rng = np.random.default_rng(20241019)
    n, small, clipped = 0, set(), set()
    for img in _images(rng):
        pil = Image.fromarray(img)
        planes = np.ascontiguousarray(img.transpose(2, 0, 1))
        small.add(img.shape[:2] if min(img.shape[:2]) <= 3 else None)
        for name, cls in PILLOW.items():
            enh = cls(pil)
            for f in FACTORS:
                f32 = float(np.float32(f))
                want = np.asarray(enh.enhance(f32))
                model = EM.apply({name: f}, planes).transpose(1, 2, 0)
                twin = fpng_amd.view_enhance_apply(fpng_amd.view_enhance(**{name: f}), planes).transpose(1, 2, 0)
                assert np.array_equal(model, want), ("model", name, f, img.shape, int(np.count_nonzero(model != want)))
                assert np.array_equal(twin, want), ("twin", name, f, img.shape, int(np.count_nonzero(twin != want)))
                if f > 1 and name != "brightness":
                    clipped |= {int(v) for v in (0, 255) if (want[img != v] == v).any()}
        n += 1
    assert n == 87 and {(h, w) for h in (1, 2, 3) for w in (1, 2, 3)} <= small and clipped == {0, 255}


def test_the_smooth_filter_is_pillows(built_lib):
    """factor 0 of Sharpness is ImageFilter.SMOOTH itself: the integer form of the model on images of every size 1 .. 12 squared"""
    from PIL import ImageFilter
    rng = np.random.default_rng(7)
    for h in range(1, 13):
        for w in range(1, 13):
            p = rng.integers(0, 256, size=(h, w), dtype=np.uint8)
            assert np.array_equal(EM.smooth(p), np.asarray(Image.fromarray(p).filter(ImageFilter.SMOOTH))), (h, w)


def test_a_factor_of_one_is_the_identity(built_lib):
    rng = np.random.default_rng(1)
    for img in _images(rng):
        planes = np.ascontiguousarray(img.transpose(2, 0, 1))
        for name in PILLOW:
            assert np.array_equal(EM.apply({name: 1.0}, planes), planes), (name, img.shape)
            assert np.array_equal(fpng_amd.view_enhance_apply(fpng_amd.view_enhance(**{name: 1.0}), planes), planes), (name, img.shape)
        assert np.array_equal(fpng_amd.view_enhance_apply(fpng_amd.view_enhance(), planes), planes)


def test_color_on_a_grey_image_is_the_identity(built_lib):
    """R = G = B = v: L = (65536 v + 0x8000) >> 16 = v, and the blend of v with v is v for every factor"""
    g = np.arange(256, dtype=np.uint8).reshape(16, 16)
    planes = np.stack([g, g, g])
    for f in FACTORS + (100.0,):
        assert np.array_equal(EM.apply({"color": f}, planes), planes), f
        assert np.array_equal(fpng_amd.view_enhance_apply(fpng_amd.view_enhance(color=f), planes), planes), f


# ---- refusals ----
@pytest.mark.parametrize("name", PLANAR + HWC)
def test_call_level_refusals_need_no_encoder(built_lib, name):
    """with a NULL encoder every call returns -1 and the message names the reason: a bad argument its own, a good set only the
    missing encoder"""
    lib = _lib.load()
    fn, hwc = getattr(lib, name), name in HWC
    fmt = _lib.FloatFormat()

    def why():
        return lib.fpng_amd_last_error().decode()

    def fresh(chans=3):  # the second record's window is 6 x 4
        files, cnt, c, v, d, col, post, res = _arrays([GOOD[0], GOOD[1], GOOD[2]], [2, 1], hwc, chans)
        return files, cnt, c, v, d, col, post, (_lib.ViewWarp * 3)(), (_lib.ViewTone * 3)(), (_lib.ViewEnhance * 3)(), res

    files, cnt, c, v, d, col, post, warp, tone, enh, res = fresh()
    for colors in (col, None):  # (NULL colors, posts, warps and tones: the identity, no flags, no warp, no op)
        for posts in (post, None):
            for warps in (warp, None):
                for tones in (tone, None):
                    assert fn(None, files, 2, cnt, c, v, d, colors, posts, warps, tones, enh, None, res) == -1 and "null/empty batch" in why(), why()
                    assert fn(None, files, 2, cnt, c, v, d, colors, posts, warps, tones, enh, C.byref(fmt), res) == -1 and "null/empty batch" in why(), why()
                    assert fn(None, files, 2, cnt, c, v, d, colors, posts, warps, tones, None, None, res) == -1 and "null enhances" in why(), why()
    # ---- the records ----
    for others in (True, False):
        rest = (post, warp, tone) if others else (None, None, None)
        for values, piece in BAD_RECORDS:
            files, cnt, c, v, d, col, post, warp, tone, enh, res = fresh()
            _fill(enh[1], values)
            assert fn(None, files, 2, cnt, c, v, d, col, *rest, enh, None, res) == -1 and piece in why(), (values, why())
        for values in GOOD_RECORDS:
            files, cnt, c, v, d, col, post, warp, tone, enh, res = fresh()
            _fill(enh[2], values)  # (the last record of the call is judged too)
            assert fn(None, files, 2, cnt, c, v, d, col, *rest, enh, None, res) == -1 and "null/empty batch" in why(), (values, why())
    files, cnt, c, v, d, col, post, warp, tone, enh, res = fresh()
    _fill(enh[2], BAD_RECORDS[0][0])
    assert fn(None, files, 2, cnt, c, v, d, col, post, warp, tone, enh, None, res) == -1 and "fpng_amd_view_enhance::op" in why(), why()
    # ---- COLOR on a destination of fewer than 3 planes; the other two ops leave that to the views call ----
    for chans in (1, 2):
        for at in (0, 2):
            files, cnt, c, v, d, col, post, warp, tone, enh, res = fresh(chans)
            _fill(enh[at], (COLOR, 1.5, (0, 0)))
            assert fn(None, files, 2, cnt, c, v, d, col, post, warp, tone, enh, None, res) == -1 and "at least 3 planes" in why(), (chans, at, why())
            _fill(enh[at], (SHARP, 1.5, (0, 0)))
            assert fn(None, files, 2, cnt, c, v, d, col, post, warp, tone, enh, None, res) == -1 and "at least 3 planes" not in why(), (chans, at, why())
    files, cnt, c, v, d, col, post, warp, tone, enh, res = fresh(4)
    _fill(enh[0], (COLOR, 1.5, (0, 0)))
    assert fn(None, files, 2, cnt, c, v, d, col, post, warp, tone, enh, None, res) == -1 and "null/empty batch" in why(), why()
    # ---- everything the tone call refuses ----
    files, cnt, c, v, d, col, post, warp, tone, enh, res = fresh()
    _fill(enh[0], (SHARP, 2.0, (0, 0)))
    _fill_tone(tone[1], (4, 0.0, (0, 0)))
    assert fn(None, files, 2, cnt, c, v, d, col, post, warp, tone, enh, None, res) == -1 and "fpng_amd_view_tone::op" in why(), why()
    _fill_tone(tone[1], (_lib.TONE_EQUALIZE, 2.0, (0, 0)))
    assert fn(None, files, 2, cnt, c, v, d, col, post, warp, tone, enh, None, res) == -1 and "without FPNG_AMD_TONE_CONTRAST" in why(), why()
    _fill_tone(tone[1], (_lib.TONE_CONTRAST, 2.0, (0, 0)))
    _fill_warp(warp[1], (4, 0, (1.0, 0.0, 0.0, 0.0, 1.0, 0.0), (0, 0, 0, 0), 0))
    assert fn(None, files, 2, cnt, c, v, d, col, post, warp, tone, enh, None, res) == -1 and "unknown fpng_amd_view_warp::flags" in why(), why()
    _fill_warp(warp[1], (1, 0, (1.0, 0.1, 0.0, 0.0, 1.0, 0.0), (1, 2, 3, 4), 0))
    _fill_post(post[1], (_lib.POST_BLUR, 4, 1.0, 0, 0, (0, 0)))
    assert fn(None, files, 2, cnt, c, v, d, col, post, warp, tone, enh, None, res) == -1 and "below the window" in why(), why()
    _fill_post(post[1], (_lib.POST_SOLARIZE, 0, 0.0, 256, 0, (0, 0)))
    assert fn(None, files, 2, cnt, c, v, d, col, post, warp, tone, enh, None, res) == -1 and "solarize_threshold" in why(), why()
    _fill_post(post[1], (_lib.POST_BLUR, 3, 1.0, 0, 0, (0, 0)))
    col[2].m[1][1] = NAN
    assert fn(None, files, 2, cnt, c, v, d, col, post, warp, tone, enh, None, res) == -1 and "fpng_amd_view_color::m" in why(), why()
    col[2].m[1][1] = 1.0
    good = [files, 2, cnt, c, v, d, col, post, warp, tone, enh, None, res]
    assert fn(None, *good) == -1 and "null/empty batch" in why(), why()
    for k in (0, 2, 3, 4, 5, 12):  # a null array
        args = list(good)
        args[k] = None
        assert fn(None, *args) == -1 and "null files, view_count, crops, views, dests or results" in why(), (k, why())
    for counts in ([0, 3], [3, 0]):
        assert fn(None, files, 2, (C.c_uint32 * 2)(*counts), c, v, d, col, post, warp, tone, enh, None, res) == -1 and "view_count of 0" in why(), (counts, why())
    v[1].filter = 2
    assert fn(None, *good) == -1 and "filter" in why(), why()
    v[1].filter = 1
    files[1].row_pitch = 4
    assert fn(None, *good) == -1 and "must be NULL / 0" in why(), why()


def test_the_host_twin_refuses_what_the_calls_refuse(built_lib):
    lib = _lib.load()
    planes = np.zeros((3, 4, 6), dtype=np.uint8)
    out = np.zeros_like(planes)
    for values, piece in BAD_RECORDS:
        rec = _lib.ViewEnhance()
        _fill(rec, values)
        with pytest.raises(fpng_amd.FpngAmdError, match=piece.replace("(", r"\(").replace(")", r"\)")):
            fpng_amd.view_enhance_apply(rec, planes)
    for values in GOOD_RECORDS:
        rec = _lib.ViewEnhance()
        _fill(rec, values)
        fpng_amd.view_enhance_apply(rec, planes)
    rec = fpng_amd.view_enhance(sharpness=2.0)
    assert lib.fpng_amd_view_enhance_apply(None, 6, 4, planes.ctypes.data, out.ctypes.data) == -1
    assert lib.fpng_amd_view_enhance_apply(C.byref(rec), 6, 4, None, out.ctypes.data) == -1
    assert lib.fpng_amd_view_enhance_apply(C.byref(rec), 6, 4, planes.ctypes.data, None) == -1
    assert lib.fpng_amd_view_enhance_apply(C.byref(rec), 0, 4, planes.ctypes.data, out.ctypes.data) == -1
    assert lib.fpng_amd_view_enhance_apply(C.byref(rec), 6, 0, planes.ctypes.data, out.ctypes.data) == -1
    assert lib.fpng_amd_view_enhance_apply(C.byref(rec), 0x80000000, 1, planes.ctypes.data, out.ctypes.data) == -1


# ---- the Python door ----
def test_view_enhance():
    r = fpng_amd.view_enhance()
    assert (r.op, r.factor, list(r.reserved)) == (0, 0.0, [0, 0])
    for op, name in NAMES.items():
        r = fpng_amd.view_enhance(**{name: 0.1})
        assert (r.op, r.factor) == (op, float(np.float32(0.1))) and r.factor != 0.1  # (rounded to fp32 once)
        r = fpng_amd.view_enhance(**{name: 0})
        assert (r.op, r.factor) == (op, 0.0)  # (a factor of 0 is an operation: the degenerate image)
        assert fpng_amd.view_enhance(**{name: np.float32(1.5)}).factor == 1.5
        for bad in (-0.5, NAN, INF, 1e39, "much", [1.0, 2.0]):
            with pytest.raises(ValueError):
                fpng_amd.view_enhance(**{name: bad})
    for bad in ({"brightness": 1.0, "color": 1.0}, {"brightness": 1.0, "sharpness": 0.0}, {"color": 2, "sharpness": 2}, {"brightness": 1, "color": 1, "sharpness": 1}):
        with pytest.raises(ValueError):
            fpng_amd.view_enhance(**bad)
    good = fpng_amd.view_enhance(sharpness=2.0)
    for bad in (lambda: fpng_amd.view_enhance_apply({"sharpness": 2.0}, np.zeros((3, 2, 2), dtype=np.uint8)), lambda: fpng_amd.view_enhance_apply(good, np.zeros((2, 2), dtype=np.uint8)),
                lambda: fpng_amd.view_enhance_apply(good, np.full((3, 2, 2), 300, dtype=np.int64)), lambda: fpng_amd.view_enhance_apply(good, np.zeros((3, 2, 2), dtype=np.float32)),
                lambda: fpng_amd.view_enhance_apply(good, np.zeros((4, 2, 2), dtype=np.uint8)), lambda: fpng_amd.view_enhance_apply(good, np.zeros((3, 0, 2), dtype=np.uint8)),
                lambda: fpng_amd.view_enhance_apply(fpng_amd.view_tone(), np.zeros((3, 2, 2), dtype=np.uint8))):
        with pytest.raises(ValueError):
            bad()


@pytest.mark.parametrize("hwc", [False, True])
def test_the_enhance_keyword_shapes_and_lengths(hwc):
    """make_decode_batch_views(_hwc)(..., enhance=) needs no GPU: one record, one per file, one per view; wrong lengths and types raise"""
    make = Encoder.make_decode_batch_views_hwc if hwc else Encoder.make_decode_batch_views
    pngs = [b"x" * 8, b"y" * 8]
    crops = [[(0, 0, 8, 8), (1, 1, 4, 4)], [(0, 0, 8, 8)]]
    outs = [[torch.empty((4, 4, 3) if hwc else (3, 4, 4), dtype=torch.uint8) for _ in cs] for cs in crops]
    a, b = fpng_amd.view_enhance(color=0.5), fpng_amd.view_enhance(sharpness=1.5)
    assert make(pngs, crops, outs, (4, 4)).enhances is None and make(pngs, crops, outs, (4, 4), post=fpng_amd.view_post(solarize=1), tone=fpng_amd.view_tone()).enhances is None
    db = make(pngs, crops, outs, (4, 4), enhance=a)
    assert db.colors is None and db.posts is None and db.warps is None and db.tones is None and [(p.op, p.factor) for p in db.enhances] == [(COLOR, 0.5)] * 3
    db = make(pngs, crops, outs, (4, 4), enhance=[a, b])
    assert [(p.op, p.factor) for p in db.enhances] == [(COLOR, 0.5), (COLOR, 0.5), (SHARP, 1.5)]
    db = make(pngs, crops, outs, (4, 4), enhance=[[b, a], [fpng_amd.view_enhance()]], color=np.eye(3, 4), post=fpng_amd.view_post(posterize=2), warp=fpng_amd.view_warp(),
              tone=fpng_amd.view_tone(equalize=True))
    assert db.colors is not None and db.posts is not None and db.warps is not None and db.tones is not None and [p.op for p in db.enhances] == [SHARP, COLOR, 0]
    for bad in ([a], [a, b, a], [[a], [b]], [[a, b, a], b], [[a, b], []], 3, [a, 3], [[a, {"color": 1.0}], b], "ab", fpng_amd.view_post(), fpng_amd.view_tone()):
        with pytest.raises(ValueError):
            make(pngs, crops, outs, (4, 4), enhance=bad)


# ---- the host twin under the sanitizers ----
def _sanitizer_planes(w, h, kind):
    x, y = np.arange(w, dtype=np.int64)[None, :], np.arange(h, dtype=np.int64)[:, None]
    if kind == 0:
        return np.stack([((7 * x + 13 * y + x * y + 50 * c) & 255) for c in range(3)]).astype(np.uint8)
    if kind == 1:
        return np.stack([np.full((h, w), 17 + c) for c in range(3)]).astype(np.uint8)
    if kind == 2:
        return np.stack([np.where((x + y) & 1, 255, c) for c in range(3)]).astype(np.uint8)
    return np.stack([100 + (x + 3 * y + c) % 7 for c in range(3)]).astype(np.uint8)


def _sanitizer_cases():
    """(w, h, kind, op, reserved, factor): every edge shape with every kind of image and every op; and records the calls refuse"""
    out = []
    sizes = [(w, h) for w in (1, 2, 3, 4, 17, 64, 65, 130) for h in (1, 2, 3, 4, 17, 33)]
    for n, (w, h) in enumerate(sizes):
        for kind in range(4):
            out.append((w, h, kind, 0, 0, 0.0))
            out += [(w, h, kind, op, 0, f) for op in (BRIGHT, COLOR, SHARP) for f in (0.0, 1.0, float(np.float32(0.37 + 0.01 * n)), 1.0 + 0.25 * kind + 0.001 * n, 99.5, 3.0e38)]
    out += [(6, 4, 0, 4, 0, 1.0), (6, 4, 0, BRIGHT, 1, 1.0), (6, 4, 1, COLOR, 0, NAN), (6, 4, 2, SHARP, 0, -1.0), (6, 4, 3, 0, 0, 2.0), (6, 4, 0, SHARP, 0, INF)]
    return out


def test_the_host_twin_under_the_sanitizers(built_lib, tmp_path):
    """tests/cpp/view_enhance_apply.cpp, a stand-alone program over view_enhance.h built with the address and undefined-behaviour
    sanitizers and run on the CPU: no report, and every view it prints is the model's"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "view_enhance_apply")
    # (-Wno-unknown-pragmas: the header's `#pragma clang fp contract`; g++ in ISO mode does not contract on x86-64.  The sanitizers'
    #  runtimes are linked into the program where the compiler has them as archives, so that it starts in any environment)
    cmd = ["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-I", os.path.join(root, "fpng_amd", "csrc"),
           "-I", os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "view_enhance_apply.cpp"), "-o", exe]
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
        ok = op <= 3 and not reserved and (math.isfinite(f) and f >= 0 if op else f == 0)
        if not ok:
            assert ln.startswith("refused "), (w, h, kind, op, f, ln[:80])
            refused += 1
            continue
        want = "ok " + EM.apply({NAMES[op]: float(np.float32(f))} if op else {}, _sanitizer_planes(w, h, kind)).tobytes().hex()
        assert ln == want, (w, h, kind, op, f)
    assert refused == 6


# ---- rotate_matrix and augment_op ----
def _through_the_twins(recs, img):
    """the (h, w, 3) image through the host twins of the records of an augment_op() dict, in the stages' order"""
    planes = np.ascontiguousarray(img.transpose(2, 0, 1))
    assert set(recs) <= {"color", "warp", "tone", "enhance", "post"} and "color" not in recs
    if "warp" in recs:
        planes = np.stack([fpng_amd.view_warp_apply(recs["warp"], p, False, recs["warp"].fill[c]) for c, p in enumerate(planes)])
    if "tone" in recs:
        planes = fpng_amd.view_tone_apply(recs["tone"], planes)
    if "enhance" in recs:
        planes = fpng_amd.view_enhance_apply(recs["enhance"], planes)
    if "post" in recs:
        planes = np.stack([fpng_amd.view_post_apply(recs["post"], p) for p in planes])
    return planes.transpose(1, 2, 0)


RESAMPLE = {"nearest": Image.NEAREST, "bilinear": Image.BILINEAR}


@pytest.mark.parametrize("filter", ["nearest", "bilinear"])
def test_rotate_matrix_is_image_rotate(built_lib, filter):
    """rotate_matrix() + view_warp_apply against Image.rotate (its transposes for 0, 180 and a square's 90 and 270 included) on a square and
    a non-square image"""
    rng = np.random.default_rng(11)
    for h, w in ((24, 24), (19, 31)):
        img = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
        pil = Image.fromarray(img)
        for angle in (0, 90, 180, 270, 30, -13.7):
            want = np.asarray(pil.rotate(angle, RESAMPLE[filter], fillcolor=(9, 99, 199)))
            got = _through_the_twins({"warp": fpng_amd.view_warp(fpng_amd.rotate_matrix(w, h, angle), filter, (9, 99, 199))}, img)
            assert np.array_equal(got, want), (h, w, angle, int(np.count_nonzero(got != want)))


def _pillow_op(name, m, pil, filter, fill):
    """what torchvision's _apply_op does to a PIL image, in Pillow's own calls (torchvision's affine() hands Image.transform the
    inverse matrix: a shear about (0, 0) is x + tan(s) y, a translation subtracts)"""
    w, h = pil.size
    if name == "Identity":
        return pil
    if name == "ShearX":
        return pil.transform((w, h), Image.AFFINE, (1.0, math.tan(math.radians(math.degrees(math.atan(m)))), 0.0, 0.0, 1.0, 0.0), RESAMPLE[filter], fillcolor=fill)
    if name == "ShearY":
        return pil.transform((w, h), Image.AFFINE, (1.0, 0.0, 0.0, math.tan(math.radians(math.degrees(math.atan(m)))), 1.0, 0.0), RESAMPLE[filter], fillcolor=fill)
    if name == "TranslateX":
        return pil.transform((w, h), Image.AFFINE, (1.0, 0.0, -float(int(m)), 0.0, 1.0, 0.0), RESAMPLE[filter], fillcolor=fill)
    if name == "TranslateY":
        return pil.transform((w, h), Image.AFFINE, (1.0, 0.0, 0.0, 0.0, 1.0, -float(int(m))), RESAMPLE[filter], fillcolor=fill)
    if name == "Rotate":
        return pil.rotate(m, RESAMPLE[filter], fillcolor=fill)
    if name in ("Brightness", "Color", "Contrast", "Sharpness"):
        return getattr(ImageEnhance, name)(pil).enhance(float(np.float32(1.0 + m)))
    if name == "Posterize":
        return ImageOps.posterize(pil, int(m))
    if name == "Solarize":
        return ImageOps.solarize(pil, m)
    return {"AutoContrast": ImageOps.autocontrast, "Equalize": ImageOps.equalize}[name](pil)


MAGNITUDES = {"Identity": (0.0,), "ShearX": (0.3, -0.99), "ShearY": (0.3, -0.99), "TranslateX": (5.0, -7.9), "TranslateY": (5.0, -7.9), "Rotate": (30.0, -135.0),
              "Brightness": (0.5, -0.99), "Color": (0.9, -0.5), "Contrast": (0.7, -0.3), "Sharpness": (0.99, -0.8), "Posterize": (4, 2.0), "Solarize": (128.0, 100.5, 0.0, 255.5),
              "AutoContrast": (0.0,), "Equalize": (0.0,)}


def test_every_augment_op_is_its_pillow_call(built_lib):
    assert set(MAGNITUDES) == set(fpng_amd.api.AUGMENT_OPS) and len(MAGNITUDES) == 14
    rng = np.random.default_rng(12)
    fill = (7, 70, 170)
    for h, w in ((21, 33), (16, 16)):
        img = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
        pil = Image.fromarray(img)
        for name, ms in MAGNITUDES.items():
            for m in ms:
                for filter in ("nearest", "bilinear"):
                    recs = fpng_amd.augment_op(name, m, w, h, filter=filter, fill=fill)
                    want = np.asarray(_pillow_op(name, m, pil, filter, fill))
                    got = _through_the_twins(recs, img)
                    assert np.array_equal(got, want), (name, m, filter, (h, w), int(np.count_nonzero(got != want)))
    assert fpng_amd.augment_op("Identity", 0.0, 8, 8) == {}
    for bad in ("Invert", "identity", "", None):
        with pytest.raises(ValueError):
            fpng_amd.augment_op(bad, 0.0, 8, 8)
