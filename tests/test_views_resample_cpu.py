"""No-GPU tests of the per-view RESAMPLE record of the views calls (fpng_amd_decode_batch(_device)_planar_views_resample /
_hwc_views_resample): Pillow's nearest, box, Hamming and Lanczos filters.  The model of resample_model.py against Pillow -- one axis
at a time over the size sweep, two axes on RGB and RGBA images, NEAREST's running sum; the host twins fpng_amd_resample_weights and
fpng_amd_resample_view_source -- the text the kernels run, sin and cos included -- against the model on the same sweep: first,
count and every weight, the sum of magnitudes, the taps at each filter's limit; the descriptors; every call-level refusal, none of
which needs an encoder or a device; what the view plan makes of the records and of the NEAREST index tables (a stand-alone
program over view_plan.h under the sanitizers)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch
from PIL import Image

import fpng_amd
from fpng_amd import _lib
from fpng_amd.api import Encoder

import alpha_model as AM
import resample_model as SM
import resize_view_model as VM
from test_resize_view_cpu import GOOD
from test_views_post_cpu import _arrays

PLANAR = ("fpng_amd_decode_batch_planar_views_resample", "fpng_amd_decode_batch_device_planar_views_resample")
HWC = ("fpng_amd_decode_batch_hwc_views_resample", "fpng_amd_decode_batch_device_hwc_views_resample")
PIL_FILTER = {"nearest": Image.NEAREST, "box": Image.BOX, "hamming": Image.HAMMING, "lanczos": Image.LANCZOS, "bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC}
NEAREST, BOX, HAMMING, LANCZOS = (SM.RESAMPLE[f] for f in SM.NEW_FILTERS)
# the sweep of the sizes of one axis: every pair inside the filter's limit
INS = list(range(1, 130)) + [255, 256, 257, 500, 1000, 1024, 2047]
OUTS = list(range(1, 100)) + [224, 256, 333]
PAIRS = {"nearest": 13514, "box": 13514, "hamming": 13514, "lanczos": 12749}
# pairs where (int)((o + 0.5) * in / out) is another table than the running sum's
PRODUCT_IS_WRONG = [(2, 7), (2, 15), (2, 21), (252, 10), (252, 13)]  # (of 31 011 such pairs with in, out < 400)


def _row(in_size, seed):
    """a one-row image whose even samples are 0 or 255: the sums reach both ends"""
    rng = np.random.default_rng(seed)
    row = rng.integers(0, 256, (1, in_size), dtype=np.uint8)
    row[:, ::2] = rng.choice(np.array([0, 255], dtype=np.uint8), row[:, ::2].shape)
    return row


def test_entry_points_and_record(built_lib):
    lib = _lib.load()
    for name in PLANAR + HWC + ("fpng_amd_resample_weights", "fpng_amd_resample_view_source"):
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
    assert lib.fpng_amd_abi_version() == 5  # (new entry points, the same ABI version)
    assert C.sizeof(_lib.ViewResample) == 16
    assert {n: getattr(_lib.ViewResample, n).offset for n, _ in _lib.ViewResample._fields_} == {"filter": 0, "flags": 4, "reserved": 8}
    assert (NEAREST, BOX, HAMMING, LANCZOS) == (_lib.RESAMPLE_NEAREST, _lib.RESAMPLE_BOX, _lib.RESAMPLE_HAMMING, _lib.RESAMPLE_LANCZOS) == (1, 2, 3, 4)
    for fn in (lib.fpng_amd_decode_batch_planar_views_resample, lib.fpng_amd_decode_batch_hwc_views_resample):
        assert fn.argtypes[7:14] == [C.POINTER(r) for r in (_lib.ViewColor, _lib.ViewPost, _lib.ViewWarp, _lib.ViewTone, _lib.ViewEnhance, _lib.ViewAlpha, _lib.ViewResample)]


# ---- 1. the sweep: the model against Pillow, the twin against the model ----
@pytest.mark.parametrize("filter", SM.NEW_FILTERS)
def test_the_sweep_of_one_axis(built_lib, filter):
    """every pair of the sweep inside the filter's limit.  The model's pass equals Pillow's resize of a one-row image; the library's
    twin equals the model in first, count and every weight (the weights behind a row's count are 0); 2^21 + 255 * sum |K| stays
    below 2^31 and no sample has more than 65 taps"""
    pairs, most, taps = 0, 0, 0
    for i in INS:
        row = _row(i, i)
        img = Image.fromarray(row)
        for o in OUTS:
            if not SM.scale_ok(i, o, filter):
                continue
            pairs += 1
            first, count, K = SM.axis_weights.__wrapped__(i, o, filter)
            got = np.clip((np.array([sum(int(row[0, f + t]) * k for t, k in enumerate(ks)) for f, ks in zip(first, K)], dtype=np.int64) + (1 << 21)) >> 22, 0, 255)
            assert np.array_equal(np.asarray(img.resize((o, 1), PIL_FILTER[filter]))[0], got), (filter, i, o)
            lf, lc, lk = fpng_amd.resample_weights(i, o, filter)
            assert lf.tolist() == first and lc.tolist() == count, (filter, i, o)
            want = np.zeros((o, _lib.RESIZE_MAX_TAPS), dtype=np.int32)
            for q, ks in enumerate(K):
                want[q, :len(ks)] = ks
            assert np.array_equal(lk, want), (filter, i, o, np.argwhere(lk != want)[:3].tolist())
            most, taps = max(most, int(np.abs(lk).sum(axis=1).max())), max(taps, max(count))
    assert pairs == PAIRS[filter]
    assert (1 << 21) + 255 * most < (1 << 31) and taps <= _lib.RESIZE_MAX_TAPS, (most / (1 << 22), taps)
    if filter == "nearest":
        assert most == 1 << 22 and taps == 1
    if filter == "lanczos":
        assert 1.5 < most / (1 << 22) < 1.58  # (the cubic's is 1.27: the bound above has room for both)


def test_hammings_constants_are_floats(monkeypatch):
    """Pillow writes the window's constants 0.54f and 0.46f.  With the doubles 0.54 and 0.46 the weights of 2822 of the sweep's pairs
    differ, and Pillow's bytes with them for two: 118 -> 60 and 118 -> 90, where the model as it stands agrees"""
    raw = SM._vm_axis_weights.__wrapped__  # (past the caches)

    def passes(i, o):
        first, _, K = raw(i, o, "hamming")
        return [min(max(((1 << 21) + sum(int(row[0, f + t]) * k for t, k in enumerate(ks))) >> 22, 0), 255) for f, ks in zip(first, K)]

    row = _row(118, 118)
    want = {o: np.asarray(Image.fromarray(row).resize((o, 1), Image.HAMMING))[0].tolist() for o in (60, 90)}
    assert all(passes(118, o) == want[o] for o in want)
    monkeypatch.setattr(SM, "_C0", 0.54)
    monkeypatch.setattr(SM, "_C1", 0.46)
    assert all(passes(118, o) != want[o] for o in want)


def test_nearest_is_the_running_sum(built_lib):
    """Pillow's NEAREST for every in <= 256 and out < 400 is the accumulated index table; the product form is another table for the
    pairs of PRODUCT_IS_WRONG (2 -> 7 is the first), where Pillow, the model and the twin agree with the sum"""
    ramp = np.arange(256, dtype=np.uint8)
    for i in range(1, 257):
        img = Image.fromarray(np.stack([ramp[:i], (ramp[:i].astype(np.int64) * 7 % 256).astype(np.uint8)]))
        for o in range(1, 400):
            idx = SM.nearest_indices(i, o)
            got = np.asarray(img.resize((o, 2), Image.NEAREST))
            assert got[0].tolist() == idx and got[1].tolist() == [k * 7 % 256 for k in idx], (i, o)
    assert SM.product_indices(2, 7) != SM.nearest_indices(2, 7)
    for i, o in PRODUCT_IS_WRONG:
        idx = SM.nearest_indices(i, o)
        assert SM.product_indices(i, o) != idx, (i, o)
        assert np.asarray(Image.fromarray(ramp[None, :i]).resize((o, 1), Image.NEAREST))[0].tolist() == idx
        first, count, K = fpng_amd.resample_weights(i, o, "nearest")
        assert first.tolist() == idx and count.tolist() == [1] * o and K[:, 0].tolist() == [1 << 22] * o and not K[:, 1:].any()


@pytest.mark.parametrize("filter", SM.NEW_FILTERS)
def test_two_axes_against_pillow(filter):
    """RGB and RGBA images, shrunk in x and grown in y as in (600, 130) -> (224, 224), and the other way round.  Pillow resizes an
    RGBA image premultiplied under the three convolutions and plane by plane under NEAREST"""
    rng = np.random.default_rng(77)
    for (w, h), full in (((600, 130), (224, 224)), ((130, 600), (224, 224)), ((257, 49), (129, 25)), ((9, 11), (65, 17)), ((96, 64), (9, 6))):
        rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        rgb[::3, ::2] = rng.choice(np.array([0, 255], dtype=np.uint8), rgb[::3, ::2].shape)
        want = np.asarray(Image.fromarray(rgb).resize(full, PIL_FILTER[filter])).transpose(2, 0, 1)
        assert np.array_equal(SM.view_planes(np.ascontiguousarray(rgb.transpose(2, 0, 1)), full, None, filter), want), (filter, w, h, full)
        rgba = AM.pattern(w, h, 5)
        want = np.asarray(Image.fromarray(rgba).resize(full, PIL_FILTER[filter])).transpose(2, 0, 1)
        alpha = {} if filter == "nearest" else {"op": "premultiplied"}
        assert np.array_equal(AM.view_planes(alpha, np.ascontiguousarray(rgba.transpose(2, 0, 1)), full, None, filter), want), (filter, w, h, full)


def test_the_older_filters_are_what_they_were():
    """importing resample_model leaves resize_view_model's answers for its own two filters alone"""
    for f in VM.FILTERS:
        assert VM.axis_weights(600, 224, f) == SM._vm_axis_weights(600, 224, f) and VM.axis_weights is SM.axis_weights
    assert VM.FILTERS == ("bilinear", "bicubic")


# ---- 2. the limits and the source box ----
def test_the_limits_taps_and_tile_bounds(built_lib):
    """exactly at each filter's limit the twin answers, with at most 65 taps; one sample past it, it refuses"""
    for filter in SM.NEW_FILTERS:
        for out in (1, 2, 3, 6, 9, 30):
            at = 32 * out // 3 if filter == "lanczos" else 32 * out
            assert SM.scale_ok(at, out, filter) and not SM.scale_ok(at + 1, out, filter)
            first, count, K = fpng_amd.resample_weights(at, out, filter)
            assert int(count.max()) <= _lib.RESIZE_MAX_TAPS and int((first + count).max()) <= at
            if filter != "nearest" and at >= 96 and 3 * at == (32 if filter == "lanczos" else 96) * out:  # (the limit met exactly, an input wider than the support: the most taps the filter has)
                assert int(count.max()) >= (32 if filter == "box" else 64)
            with pytest.raises(fpng_amd.FpngAmdError, match="Lanczos" if filter == "lanczos" else "nearest, box, Hamming"):
                fpng_amd.resample_weights(at + 1, out, filter)
        for bad in ((0, 1), (1, 0)):
            with pytest.raises(fpng_amd.FpngAmdError):
                fpng_amd.resample_weights(*bad, filter)
    lib = _lib.load()
    one, w = (C.c_uint32 * 1)(), (C.c_int32 * 65)()
    for bad in (0, 5, 0xFFFFFFFF):
        assert lib.fpng_amd_resample_weights(4, 1, bad, one, one, w) == -1 and b"unknown filter" in lib.fpng_amd_last_error()
    assert lib.fpng_amd_resample_weights(4, 1, BOX, None, one, w) == -1 and lib.fpng_amd_resample_weights(4, 1, BOX, one, one, None) == -1


def test_the_source_box(built_lib):
    """fpng_amd_resample_view_source against the model: the views the GPU tests decode, every window of two small shapes, and a
    record without a filter (fpng_amd_resize_view_source's answer)"""
    for dims, views in SM.VIEWS.items():
        for crop, full, window, filters in views:
            for f in filters:
                for own in VM.FILTERS:
                    assert fpng_amd.resample_view_source(crop, full, window, own, f) == SM.view_source(crop, full, window, f), (crop, full, window, f)
    for f in SM.NEW_FILTERS:
        for crop, full in (((3, 4, 23, 9), (7, 20)), ((0, 0, 5, 64), (11, 6))):
            for x in range(full[0]):
                for w in (1, 2, full[0] - x):
                    if x + w <= full[0]:
                        window = (x, full[1] // 2, w, full[1] - full[1] // 2)
                        assert fpng_amd.resample_view_source(crop, full, window, "bilinear", f) == SM.view_source(crop, full, window, f), (crop, full, window, f)
    for own in VM.FILTERS:
        args = ((2, 3, 96, 64), (24, 16), (5, 3, 7, 8), own)
        assert fpng_amd.resample_view_source(*args, None) == fpng_amd.resize_view_source(*args) == VM.view_source(*args)
        assert fpng_amd.resample_view_source(*args, fpng_amd.view_resample("box")) == SM.view_source(*args[:3], "box")


# ---- 3. refusals ----
def _fill(rec, values):
    rec.filter, rec.flags = values[:2]
    rec.reserved[0], rec.reserved[1] = values[2]


LZ = ((0, 0, 96, 64), (9, 6, 0, 0, 9, 6, 1, 1))  # a view inside every filter's limit: 3 * 96 = 32 * 9
# (filter, flags, reserved) and a piece of the message
BAD_RECORDS = [((5, 0, (0, 0)), "unknown fpng_amd_view_resample::filter"), ((0xFFFFFFFF, 0, (0, 0)), "unknown fpng_amd_view_resample::filter"),
               ((NEAREST, 1, (0, 0)), "fpng_amd_view_resample::flags must be 0"), ((0, 0x80000000, (0, 0)), "fpng_amd_view_resample::flags must be 0"),
               ((BOX, 0, (1, 0)), "fpng_amd_view_resample::reserved must be 0"), ((0, 0, (0, 7)), "fpng_amd_view_resample::reserved must be 0")]
GOOD_RECORDS = [(0, 0, (0, 0)), (NEAREST, 0, (0, 0)), (BOX, 0, (0, 0)), (HAMMING, 0, (0, 0)), (LANCZOS, 0, (0, 0))]


@pytest.mark.parametrize("name", PLANAR + HWC)
def test_call_level_refusals_need_no_encoder(built_lib, name):
    """with a NULL encoder every call returns -1 and the message names the reason: a bad argument its own, a good set only the
    missing encoder"""
    lib = _lib.load()
    fn, hwc = getattr(lib, name), name in HWC

    def why():
        return lib.fpng_amd_last_error().decode()

    def fresh(records=(GOOD[0], GOOD[1], GOOD[2]), chans=4):
        files, cnt, c, v, d, col, post, res = _arrays(list(records), [2, 1], hwc, chans)
        return files, cnt, c, v, d, col, post, (_lib.ViewWarp * 3)(), (_lib.ViewTone * 3)(), (_lib.ViewEnhance * 3)(), (_lib.ViewAlpha * 3)(), (_lib.ViewResample * 3)(), res

    files, cnt, c, v, d, col, post, warp, tone, enh, alp, rsm, res = fresh()
    for others in ((col, post, warp, tone, enh, alp), (None,) * 6, (col, None, None, None, None, alp)):  # (NULL: the identity, no flags, no ops)
        assert fn(None, files, 2, cnt, c, v, d, *others, rsm, None, res) == -1 and "null/empty batch" in why(), why()
        assert fn(None, files, 2, cnt, c, v, d, *others, None, None, res) == -1 and "null resamples" in why(), why()
    # ---- the records: every one of the call is judged ----
    for others in ((col, post, warp, tone, enh, alp), (None,) * 6):
        for at in (0, 1, 2):
            for values, piece in BAD_RECORDS:
                files, cnt, c, v, d, col, post, warp, tone, enh, alp, rsm, res = fresh()
                _fill(rsm[at], values)
                assert fn(None, files, 2, cnt, c, v, d, *((col, post, warp, tone, enh, alp) if others[0] is not None else others), rsm, None, res) == -1 and piece in why(), (values, why())
            for values in GOOD_RECORDS:
                files, cnt, c, v, d, col, post, warp, tone, enh, alp, rsm, res = fresh((LZ, LZ, LZ))
                _fill(rsm[at], values)
                assert fn(None, files, 2, cnt, c, v, d, col, post, warp, tone, enh, alp, rsm, None, res) == -1 and "null/empty batch" in why(), (values, why())
    # ---- NEAREST with PREMULTIPLIED ----
    for f, ok in ((NEAREST, False), (BOX, True), (HAMMING, True), (LANCZOS, True), (0, True)):
        files, cnt, c, v, d, col, post, warp, tone, enh, alp, rsm, res = fresh((LZ, LZ, LZ))
        rsm[2].filter, alp[2].op, alp[0].op = f, _lib.ALPHA_PREMULTIPLIED, _lib.ALPHA_PREMULTIPLIED
        rc = fn(None, files, 2, cnt, c, v, d, None, None, None, None, None, alp, rsm, None, res)
        assert rc == -1 and (("null/empty batch" in why()) if ok else ("PREMULTIPLIED" in why() and "NEAREST" in why())), (f, why())
    files, cnt, c, v, d, col, post, warp, tone, enh, alp, rsm, res = fresh()
    rsm[1].filter, alp[1].op = NEAREST, _lib.ALPHA_COMPOSITE  # (COMPOSITE goes with every filter)
    assert fn(None, files, 2, cnt, c, v, d, None, None, None, None, None, alp, rsm, None, res) == -1 and "null/empty batch" in why(), why()
    # ---- the limits: the crop against the full size, under the effective filter ----
    for f, (cw, ch), full, piece in ((NEAREST, (96, 64), (3, 2), None), (NEAREST, (97, 64), (3, 2), "nearest, box, Hamming"), (BOX, (96, 65), (3, 2), "nearest, box, Hamming"),
                                     (BOX, (96, 64), (3, 2), None), (HAMMING, (96, 64), (3, 2), None), (HAMMING, (97, 64), (3, 2), "nearest, box, Hamming"),
                                     (LANCZOS, (96, 64), (9, 6), None), (LANCZOS, (97, 64), (9, 6), "Lanczos limit"), (LANCZOS, (96, 65), (9, 6), "Lanczos limit"),
                                     (LANCZOS, (96, 64), (3, 2), "Lanczos limit"), (0, (96, 64), (3, 2), "bicubic: w <= 16"), (0, (96, 64), (6, 4), None)):
        view = ((0, 0, cw, ch), (full[0], full[1], 0, 0, full[0], full[1], 0, 1))  # (the view's own filter is bicubic, 16 x: the record's filter has the say)
        files, cnt, c, v, d, col, post, warp, tone, enh, alp, rsm, res = fresh((GOOD[1], view, GOOD[2]))
        rsm[1].filter = f
        assert fn(None, files, 2, cnt, c, v, d, None, None, None, None, None, None, rsm, None, res) == -1 and (piece or "null/empty batch") in why(), (f, cw, ch, full, why())
    # ---- the view's own filter must still be a valid one; everything the alpha call refuses ----
    files, cnt, c, v, d, col, post, warp, tone, enh, alp, rsm, res = fresh()
    rsm[1].filter = BOX
    good = [files, 2, cnt, c, v, d, col, post, warp, tone, enh, alp, rsm, None, res]
    assert fn(None, *good) == -1 and "null/empty batch" in why(), why()
    v[1].filter = 2
    assert fn(None, *good) == -1 and "unknown filter (FPNG_AMD_FILTER_BILINEAR, _BICUBIC)" in why(), why()
    v[1].filter = 1
    alp[0].op = 3
    assert fn(None, *good) == -1 and "fpng_amd_view_alpha::op" in why(), why()
    alp[0].op = 0
    enh[1].op = 4
    assert fn(None, *good) == -1 and "fpng_amd_view_enhance::op" in why(), why()
    enh[1].op = 0
    col[2].m[1][1] = float("nan")
    assert fn(None, *good) == -1 and "fpng_amd_view_color::m" in why(), why()
    col[2].m[1][1] = 1.0
    for k in (0, 2, 3, 4, 5, 14):  # a null array
        args = list(good)
        args[k] = None
        assert fn(None, *args) == -1 and "null files, view_count, crops, views, dests or results" in why(), (k, why())
    for counts in ([0, 3], [3, 0]):
        assert fn(None, files, 2, (C.c_uint32 * 2)(*counts), *good[3:]) == -1 and "view_count of 0" in why(), (counts, why())
    files[1].row_pitch = 4
    assert fn(None, *good) == -1 and "must be NULL / 0" in why(), why()


def test_the_source_twin_refuses_what_the_calls_refuse(built_lib):
    lib = _lib.load()
    crop, view, box = _lib.Crop(0, 0, 96, 64), _lib.ResizeView(6, 4, 0, 0, 6, 4, 0, 0), _lib.Crop()
    for values, piece in BAD_RECORDS:
        rec = _lib.ViewResample()
        _fill(rec, values)
        assert lib.fpng_amd_resample_view_source(C.byref(crop), C.byref(view), C.byref(rec), C.byref(box)) == -1 and piece.encode() in lib.fpng_amd_last_error()
    rec = fpng_amd.view_resample("lanczos")
    assert lib.fpng_amd_resample_view_source(C.byref(crop), C.byref(view), C.byref(rec), C.byref(box)) == -1 and b"Lanczos limit" in lib.fpng_amd_last_error()
    rec = fpng_amd.view_resample("hamming")
    assert lib.fpng_amd_resample_view_source(C.byref(crop), C.byref(view), C.byref(rec), C.byref(box)) == 0
    for k in range(4):
        args = [C.byref(crop), C.byref(view), C.byref(rec), C.byref(box)]
        args[k] = None
        assert lib.fpng_amd_resample_view_source(*args) == -1


# ---- 4. the Python door ----
def test_view_resample():
    assert [fpng_amd.view_resample(f).filter for f in (None, "nearest", "box", "hamming", "lanczos", 3, np.uint32(9))] == [0, NEAREST, BOX, HAMMING, LANCZOS, 3, 9]
    r = fpng_amd.view_resample()
    assert (r.filter, r.flags, list(r.reserved)) == (0, 0, [0, 0])
    for bad in ("bilinear", "bicubic", "NEAREST", -1, 1.5, True, (1,), 1 << 32):
        with pytest.raises(ValueError):
            fpng_amd.view_resample(bad)


@pytest.mark.parametrize("hwc", [False, True])
def test_the_resample_keyword_shapes_and_lengths(hwc):
    """make_decode_batch_views(_hwc)(..., resample=) needs no GPU: one name or record per call, per file, per view; wrong lengths and
    types raise; views_entry picks the new family only with resample=, and its other answers are what they were"""
    from fpng_amd.api import views_entry
    make = Encoder.make_decode_batch_views_hwc if hwc else Encoder.make_decode_batch_views
    layout = "hwc" if hwc else "planar"
    pngs = [b"x" * 8, b"y" * 8]
    crops = [[(0, 0, 8, 8), (1, 1, 4, 4)], [(0, 0, 8, 8)]]
    outs = [[torch.empty((4, 4, 3) if hwc else (3, 4, 4), dtype=torch.uint8) for _ in cs] for cs in crops]
    a = fpng_amd.view_alpha("composite", (255, 255, 255))
    db = make(pngs, crops, outs, (4, 4), alpha=a)
    assert db.resamples is None and views_entry(layout, False, db)[0] == f"fpng_amd_decode_batch_{layout}_views_alpha" and len(views_entry(layout, False, db)[1]) == 14
    assert views_entry(layout, False, make(pngs, crops, outs, (4, 4)))[0] == f"fpng_amd_decode_batch_{layout}_views"
    assert views_entry(layout, True, make(pngs, crops, outs, (4, 4), enhance=fpng_amd.view_enhance(color=0.5)))[0] == f"fpng_amd_decode_batch_device_{layout}_views_enhance"
    db = make(pngs, crops, outs, (4, 4), resample="nearest")
    assert db.colors is None and db.posts is None and db.warps is None and db.tones is None and db.enhances is None and db.alphas is None
    assert [(p.filter, p.flags, list(p.reserved)) for p in db.resamples] == [(NEAREST, 0, [0, 0])] * 3
    assert [z.filter for z in db.views] == [_lib.FILTER_BILINEAR] * 3  # (the view's own filter stays what filter= says)
    symbol, args = views_entry(layout, False, db)
    assert symbol == f"fpng_amd_decode_batch_{layout}_views_resample" and args[6:12] == [None] * 6 and args[12] is db.resamples and len(args) == 15
    db = make(pngs, crops, outs, (4, 4), filter="bicubic", resample=["box", fpng_amd.view_resample("lanczos")])
    assert [p.filter for p in db.resamples] == [BOX, BOX, LANCZOS] and [z.filter for z in db.views] == [_lib.FILTER_BICUBIC] * 3
    db = make(pngs, crops, outs, (4, 4), resample=[["hamming", None], [fpng_amd.view_resample("nearest")]], alpha=a, color=np.eye(3, 4))
    assert [p.filter for p in db.resamples] == [HAMMING, 0, NEAREST] and db.alphas is not None and db.colors is not None
    symbol, args = views_entry(layout, True, db)
    assert symbol == f"fpng_amd_decode_batch_device_{layout}_views_resample" and args[6] is db.colors and args[11] is db.alphas and args[12] is db.resamples
    for bad in (["box"], ["box", "box", "box"], [["box"], ["box"]], [["box", "box", "box"], "box"], [["box", "box"], []], 1.5, ["box", 1.5], "cubic", [["box", "linear"], None],
                fpng_amd.view_post(), a, [a, a]):
        with pytest.raises(ValueError):
            make(pngs, crops, outs, (4, 4), resample=bad)


# ---- 5. what the plan makes of the records ----
def test_the_view_plan_carries_the_records_and_the_index_tables(built_lib, tmp_path):
    """tests/cpp/view_plan_resample.cpp, a stand-alone program over view_plan.h, built with the address and undefined-behaviour
    sanitizers and run as its own process on the CPU: the effective filter and its bounds in the records, the files' boxes, the
    NEAREST index tables inside the set-up block, no report"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "view_plan_resample")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cmd = ["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(root, "fpng_amd", "csrc"),
           "-I", os.path.join(root, "include"), "-I", os.path.join(rocm, "include"), os.path.join(root, "tests", "cpp", "view_plan_resample.cpp"), "-o", exe]
    r = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if r.returncode != 0:
        r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert run.returncode == 0 and not run.stderr, (run.returncode, run.stdout[-2000:], run.stderr[-2000:])
    assert run.stdout.splitlines() == ["ok planar", "ok hwc"]
