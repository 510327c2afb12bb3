"""No-GPU tests of the per-view alpha record of the views calls (fpng_amd_decode_batch(_device)_planar_views_alpha /
_hwc_views_alpha): the exact model of alpha_model.py and the host twins fpng_amd_view_alpha_source / fpng_amd_view_alpha_result --
the text the resize kernels run in their load and their store -- against Pillow: M, U and C exhaustively, whole views against
Image.alpha_composite and Image.resize of RGBA images bit for bit; the twins against the model; every call-level refusal, none of
which needs an encoder or a device; the Python door; what the view plan makes of the records (a stand-alone program over
view_plan.h); and the conditions that the GPU test's images have to meet."""
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
from test_resize_view_cpu import GOOD
from test_views_enhance_cpu import _fill as _fill_enhance
from test_views_post_cpu import _arrays

PLANAR = ("fpng_amd_decode_batch_planar_views_alpha", "fpng_amd_decode_batch_device_planar_views_alpha")
HWC = ("fpng_amd_decode_batch_hwc_views_alpha", "fpng_amd_decode_batch_device_hwc_views_alpha")
COMPOSITE, PREMULTIPLIED = _lib.ALPHA_COMPOSITE, _lib.ALPHA_PREMULTIPLIED
RESAMPLE = {"bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC}
# (op, background, reserved) and a piece of the message
BAD_RECORDS = [((3, (0, 0, 0, 0), (0, 0)), "fpng_amd_view_alpha::op"), ((0xFFFFFFFF, (0, 0, 0, 0), (0, 0)), "fpng_amd_view_alpha::op"),
               ((COMPOSITE, (1, 2, 3, 0), (1, 0)), "reserved"), ((0, (0, 0, 0, 0), (0, 7)), "reserved"),
               ((COMPOSITE, (1, 2, 3, 4), (0, 0)), "background[3]"), ((COMPOSITE, (0, 0, 0, 255), (0, 0)), "background[3]"), ((0, (0, 0, 0, 1), (0, 0)), "background[3]"),
               ((0, (1, 0, 0, 0), (0, 0)), "without FPNG_AMD_ALPHA_COMPOSITE"), ((PREMULTIPLIED, (0, 0, 9, 0), (0, 0)), "without FPNG_AMD_ALPHA_COMPOSITE"),
               ((PREMULTIPLIED, (0, 255, 0, 0), (0, 0)), "without FPNG_AMD_ALPHA_COMPOSITE")]
GOOD_RECORDS = [(0, (0, 0, 0, 0), (0, 0)), (COMPOSITE, (0, 0, 0, 0), (0, 0)), (COMPOSITE, (255, 128, 1, 0), (0, 0)), (PREMULTIPLIED, (0, 0, 0, 0), (0, 0))]
ALPHAS = [{}, {"op": "composite", "background": (255, 255, 255)}, {"op": "composite", "background": (0, 0, 0)}, {"op": "composite", "background": (12, 200, 77)},
          {"op": "premultiplied"}]


def _fill(rec, values):
    rec.op = values[0]
    for k in range(4):
        rec.background[k] = values[1][k]
    rec.reserved[0], rec.reserved[1] = values[2]


def _planes(img):
    return np.ascontiguousarray(np.asarray(img).transpose(2, 0, 1))


def test_entry_points_and_record(built_lib):
    lib = _lib.load()
    for name in PLANAR + HWC + ("fpng_amd_view_alpha_source", "fpng_amd_view_alpha_result"):
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
    assert lib.fpng_amd_abi_version() == 5  # (new entry points, the same ABI version)
    assert C.sizeof(_lib.ViewAlpha) == 16
    assert {n: getattr(_lib.ViewAlpha, n).offset for n, _ in _lib.ViewAlpha._fields_} == {"op": 0, "background": 4, "reserved": 8}
    assert (COMPOSITE, PREMULTIPLIED) == (1, 2)
    for fn in (lib.fpng_amd_decode_batch_planar_views_alpha, lib.fpng_amd_decode_batch_hwc_views_alpha):
        assert fn.argtypes[7:13] == [C.POINTER(r) for r in (_lib.ViewColor, _lib.ViewPost, _lib.ViewWarp, _lib.ViewTone, _lib.ViewEnhance, _lib.ViewAlpha)]


# ---- 1. against Pillow ----
def _grid():
    """v along x, a along y: all 2^16 pairs"""
    v, a = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8))
    return np.ascontiguousarray(v), np.ascontiguousarray(a)


def test_premultiply_and_its_inverse_are_pillows_for_every_pair(built_lib):
    """M is convert("RGBa") of an RGBA image and U is convert("RGBA") of an RGBa image, for all 2^16 (v, a): the model and the twins"""
    v, a = _grid()
    rgba = np.stack([v, v, v, a], axis=-1)
    want_m = np.asarray(Image.fromarray(rgba, "RGBA").convert("RGBa"))
    want_u = np.asarray(Image.frombytes("RGBa", (256, 256), rgba.tobytes()).convert("RGBA"))
    assert np.array_equal(want_m[..., 3], a) and np.array_equal(want_u[..., 3], a)
    pre = fpng_amd.view_alpha("premultiplied")
    src, res = fpng_amd.view_alpha_source(pre, _planes(rgba)), fpng_amd.view_alpha_result(pre, _planes(rgba))
    for c in range(3):
        assert np.array_equal(AM.M(v, a), want_m[..., c]) and np.array_equal(AM.U(v, a), want_u[..., c])
        assert np.array_equal(src[c], want_m[..., c]) and np.array_equal(res[c], want_u[..., c])
    assert np.array_equal(src[3], a) and np.array_equal(res[3], a)
    # (the clip is live where v > a > 0, and a == 0 copies a colour that is not 0)
    assert (AM.U(v, a)[(v > a) & (a > 0)] == 255).all() and np.array_equal(AM.U(v, a)[0], v[0])


def test_compositing_is_pillows_for_every_triple(built_lib):
    """C against Image.alpha_composite over an opaque background and against Image.paste(im, mask=alpha), one 256 x 256 image of all
    (v, a) per background value: all 2^24 triples, the model and the twin"""
    v, a = _grid()
    rgba = np.stack([v, v, v, a], axis=-1)
    im = Image.fromarray(rgba, "RGBA")
    p4 = _planes(rgba)
    for b in range(256):
        over = np.asarray(Image.alpha_composite(Image.new("RGBA", im.size, (b, b, b, 255)), im))
        pasted = Image.new("RGB", im.size, (b, b, b))
        pasted.paste(im, mask=im.getchannel("A"))
        want = over[..., 0]
        assert (over[..., 3] == 255).all() and np.array_equal(np.asarray(pasted)[..., 0], want), b
        assert np.array_equal(AM.C(v, a, b), want), b
        twin = fpng_amd.view_alpha_source(fpng_amd.view_alpha("composite", (b, 255 - b, b)), p4)
        assert np.array_equal(twin[0], want) and np.array_equal(twin[2], want) and (twin[3] == 255).all(), b
        assert np.array_equal(twin[1], AM.C(v, a, 255 - b)), b
        assert np.array_equal(want[0], np.full(256, b)) and np.array_equal(want[255], v[255])  # (a == 0 gives b, a == 255 gives v)


def _images():
    rng = np.random.default_rng(20261019)
    yield AM.pattern(33, 9)
    yield AM.pattern(90, 40, 1)
    yield rng.integers(0, 256, (53, 37, 4), dtype=np.uint8)  # (noise with mixed alpha)
    yield rng.choice(np.array([0, 1, 127, 254, 255], dtype=np.uint8), size=(21, 50, 4))


# (crop, full, window) as fractions of the image: whole, upscaled and downscaled in both axes, one axis kept, with and without a
# window.  (Not full == the crop's size: Image.resize then returns a copy and never premultiplies; the rule always does.)
def _views(w, h):
    crop = (w // 7, h // 5, w - w // 3, h - h // 4)
    return [((0, 0, w, h), (2 * w + 4, 2 * h + 2), None), ((0, 0, w, h), (max(w // 3, 1), max(h // 2, 1)), None), ((0, 0, w, h), (w + 1, h), None),
            (crop, (3 * crop[2] // 2, max(crop[3] // 2, 1)), (crop[2] // 4, 0, crop[2], max(crop[3] // 2, 1))), (crop, (max(crop[2] // 2, 1), 3 * crop[3]), (0, crop[3], max(crop[2] // 2, 1), crop[3]))]


def test_whole_views_are_pillows(built_lib):
    """PREMULTIPLIED: im.crop(box).resize(full, f).crop(window) of the RGBA image; COMPOSITE: alpha_composite over the background,
    convert("RGB"), then the same chain -- both filters, upscaling and downscaling, whole images and windows of crops.  The model
    composes its own M, U, C with resize_view_model's resize; the twins around that resize give the same"""
    n = 0
    for img in _images():
        h, w = img.shape[:2]
        im = Image.fromarray(img, "RGBA")
        for crop, full, window in _views(w, h):
            x, y, cw, ch = crop
            box = (x, y, x + cw, y + ch)
            wx, wy, ww, wh = (0, 0) + full if window is None else window
            px4 = _planes(img)[:, y:y + ch, x:x + cw]
            for f, resample in RESAMPLE.items():
                for alpha in ALPHAS[1:]:
                    if alpha["op"] == "premultiplied":
                        want = np.asarray(im.crop(box).resize(full, resample).crop((wx, wy, wx + ww, wy + wh)))
                    else:
                        flat = Image.alpha_composite(Image.new("RGBA", im.size, tuple(alpha["background"]) + (255,)), im).convert("RGB")
                        want = np.asarray(flat.crop(box).resize(full, resample).crop((wx, wy, wx + ww, wy + wh)))
                        want = np.concatenate([want, np.full(want.shape[:2] + (1,), 255, np.uint8)], axis=-1)
                    got = AM.view_planes(alpha, px4, full, window, f).transpose(1, 2, 0)
                    assert np.array_equal(got, want), (img.shape, crop, full, window, f, alpha, int(np.count_nonzero(got != want)))
                    rec = fpng_amd.view_alpha(**alpha)
                    mid = AM.VM.view_planes(fpng_amd.view_alpha_source(rec, px4), full, window, f)
                    assert np.array_equal(fpng_amd.view_alpha_result(rec, mid).transpose(1, 2, 0), want), (img.shape, crop, full, window, f, alpha)
                    n += 1
    assert n == 4 * 5 * 2 * 4


def test_the_per_band_resize_is_not_pillows_rgba_resize():
    """why the stage exists: on the 37 x 53 noise image the views call's rule -- every plane on its own -- differs from Image.resize of
    the RGBA image in most samples"""
    img = list(_images())[2]
    px4 = _planes(img)
    want = AM.view_planes({"op": "premultiplied"}, px4, (20, 11), None, "bilinear")
    plain = AM.view_planes({}, px4, (20, 11), None, "bilinear")
    assert np.count_nonzero((want != plain).any(axis=0)) > 200


# ---- 2. the twins against the model ----
def test_the_twins_are_the_model_on_random_planes(built_lib):
    rng = np.random.default_rng(5)
    for k in range(40):
        h, w = (int(v) for v in rng.integers(1, 48, size=2))
        px = rng.integers(0, 256, (4, h, w), dtype=np.uint8)
        if k % 3 == 0:
            px[3] = rng.choice(np.array([0, 1, 254, 255], dtype=np.uint8), size=(h, w))
        for alpha in ALPHAS:
            rec = fpng_amd.view_alpha(**alpha)
            assert np.array_equal(fpng_amd.view_alpha_source(rec, px), AM.source(alpha, px)), (k, alpha)
            assert np.array_equal(fpng_amd.view_alpha_result(rec, px), AM.result(alpha, px)), (k, alpha)
        assert np.array_equal(fpng_amd.view_alpha_source(fpng_amd.view_alpha(), px), px) and np.array_equal(fpng_amd.view_alpha_result(fpng_amd.view_alpha(), px), px)


def test_an_opaque_alpha_plane_makes_every_op_the_identity(built_lib):
    """C(v, 255, b) = M(v, 255) = U(v, 255) = v: what a 3-channel file, whose fourth plane is 255, gets from any record"""
    v = np.arange(256, dtype=np.uint8)
    for b in (0, 1, 128, 255):
        assert np.array_equal(AM.C(v, 255, b), v)
    assert np.array_equal(AM.M(v, 255), v) and np.array_equal(AM.U(v, 255), v)
    rng = np.random.default_rng(9)
    px = rng.integers(0, 256, (4, 7, 11), dtype=np.uint8)
    px[3] = 255
    for alpha in ALPHAS:
        rec = fpng_amd.view_alpha(**alpha)
        assert np.array_equal(fpng_amd.view_alpha_source(rec, px), px) and np.array_equal(fpng_amd.view_alpha_result(rec, px), px), alpha
        assert np.array_equal(AM.view_planes(alpha, px, (5, 9), None, "bicubic"), AM.view_planes({}, px, (5, 9), None, "bicubic")), alpha


# ---- 3. refusals ----
@pytest.mark.parametrize("name", PLANAR + HWC)
def test_call_level_refusals_need_no_encoder(built_lib, name):
    """with a NULL encoder every call returns -1 and the message names the reason: a bad argument its own, a good set only the
    missing encoder"""
    lib = _lib.load()
    fn, hwc = getattr(lib, name), name in HWC
    fmt = _lib.FloatFormat()

    def why():
        return lib.fpng_amd_last_error().decode()

    def fresh(chans=4):
        files, cnt, c, v, d, col, post, res = _arrays([GOOD[0], GOOD[1], GOOD[2]], [2, 1], hwc, chans)
        return files, cnt, c, v, d, col, post, (_lib.ViewWarp * 3)(), (_lib.ViewTone * 3)(), (_lib.ViewEnhance * 3)(), (_lib.ViewAlpha * 3)(), res

    files, cnt, c, v, d, col, post, warp, tone, enh, alp, res = fresh()
    for colors in (col, None):  # (NULL colors, posts, warps, tones and enhances: the identity, no flags, no warp, no ops)
        for posts in (post, None):
            for warps in (warp, None):
                for tones in (tone, None):
                    for enhs in (enh, None):
                        assert fn(None, files, 2, cnt, c, v, d, colors, posts, warps, tones, enhs, alp, None, res) == -1 and "null/empty batch" in why(), why()
                        assert fn(None, files, 2, cnt, c, v, d, colors, posts, warps, tones, enhs, alp, C.byref(fmt), res) == -1 and "null/empty batch" in why(), why()
                        assert fn(None, files, 2, cnt, c, v, d, colors, posts, warps, tones, enhs, None, None, res) == -1 and "null alphas" in why(), why()
    # ---- the records ----
    for others in (True, False):
        rest = (col, post, warp, tone, enh) if others else (None,) * 5
        for at in (0, 1, 2):  # (every record of the call is judged, the last one too)
            for values, piece in BAD_RECORDS:
                files, cnt, c, v, d, col, post, warp, tone, enh, alp, res = fresh()
                _fill(alp[at], values)
                assert fn(None, files, 2, cnt, c, v, d, *rest, alp, None, res) == -1 and piece in why(), (values, why())
            for values in GOOD_RECORDS:
                files, cnt, c, v, d, col, post, warp, tone, enh, alp, res = fresh(3 + (at & 1))
                _fill(alp[at], values)
                assert fn(None, files, 2, cnt, c, v, d, *rest, alp, None, res) == -1 and "null/empty batch" in why(), (values, why())
    # ---- everything the enhance call refuses ----
    files, cnt, c, v, d, col, post, warp, tone, enh, alp, res = fresh()
    _fill(alp[0], GOOD_RECORDS[2])
    _fill_enhance(enh[1], (4, 1.0, (0, 0)))
    assert fn(None, files, 2, cnt, c, v, d, col, post, warp, tone, enh, alp, None, res) == -1 and "fpng_amd_view_enhance::op" in why(), why()
    _fill_enhance(enh[1], (0, 1.0, (0, 0)))
    assert fn(None, files, 2, cnt, c, v, d, col, post, warp, tone, enh, alp, None, res) == -1 and "must be 0 without an op" in why(), why()
    _fill_enhance(enh[1], (_lib.ENHANCE_SHARPNESS, 1.5, (0, 0)))
    tone[2].op = 4
    assert fn(None, files, 2, cnt, c, v, d, col, post, warp, tone, enh, alp, None, res) == -1 and "fpng_amd_view_tone::op" in why(), why()
    tone[2].op = 0
    warp[0].flags = 4
    assert fn(None, files, 2, cnt, c, v, d, col, post, warp, tone, enh, alp, None, res) == -1 and "unknown fpng_amd_view_warp::flags" in why(), why()
    warp[0].flags = 0
    post[1].flags = 8
    assert fn(None, files, 2, cnt, c, v, d, col, post, warp, tone, enh, alp, None, res) == -1 and "fpng_amd_view_post::flags" in why(), why()
    post[1].flags = 0
    col[2].m[1][1] = float("nan")
    assert fn(None, files, 2, cnt, c, v, d, col, post, warp, tone, enh, alp, None, res) == -1 and "fpng_amd_view_color::m" in why(), why()
    col[2].m[1][1] = 1.0
    good = [files, 2, cnt, c, v, d, col, post, warp, tone, enh, alp, None, res]
    assert fn(None, *good) == -1 and "null/empty batch" in why(), why()
    for k in (0, 2, 3, 4, 5, 13):  # a null array
        args = list(good)
        args[k] = None
        assert fn(None, *args) == -1 and "null files, view_count, crops, views, dests or results" in why(), (k, why())
    for counts in ([0, 3], [3, 0]):
        assert fn(None, files, 2, (C.c_uint32 * 2)(*counts), c, v, d, col, post, warp, tone, enh, alp, None, res) == -1 and "view_count of 0" in why(), (counts, why())
    v[1].filter = 2
    assert fn(None, *good) == -1 and "filter" in why(), why()
    v[1].filter = 1
    if hwc:
        d[0].flags = 2
        assert fn(None, *good) == -1 and "fpng_amd_view_dest_hwc::flags" in why(), why()
        d[0].flags = 0
    files[1].row_pitch = 4
    assert fn(None, *good) == -1 and "must be NULL / 0" in why(), why()


def test_the_host_twins_refuse_what_the_calls_refuse(built_lib):
    lib = _lib.load()
    planes = np.zeros((4, 4, 6), dtype=np.uint8)
    out = np.zeros_like(planes)
    for twin, fn in ((fpng_amd.view_alpha_source, lib.fpng_amd_view_alpha_source), (fpng_amd.view_alpha_result, lib.fpng_amd_view_alpha_result)):
        for values, piece in BAD_RECORDS:
            rec = _lib.ViewAlpha()
            _fill(rec, values)
            with pytest.raises(fpng_amd.FpngAmdError, match=piece.replace("[", r"\[").replace("]", r"\]")):
                twin(rec, planes)
        for values in GOOD_RECORDS:
            rec = _lib.ViewAlpha()
            _fill(rec, values)
            twin(rec, planes)
        rec = fpng_amd.view_alpha("premultiplied")
        assert fn(None, 6, 4, planes.ctypes.data, out.ctypes.data) == -1
        assert fn(C.byref(rec), 6, 4, None, out.ctypes.data) == -1
        assert fn(C.byref(rec), 6, 4, planes.ctypes.data, None) == -1
        assert fn(C.byref(rec), 0, 4, planes.ctypes.data, out.ctypes.data) == -1
        assert fn(C.byref(rec), 6, 0, planes.ctypes.data, out.ctypes.data) == -1


# ---- the Python door ----
def test_view_alpha():
    r = fpng_amd.view_alpha()
    assert (r.op, list(r.background), list(r.reserved)) == (0, [0, 0, 0, 0], [0, 0])
    r = fpng_amd.view_alpha("composite")
    assert (r.op, list(r.background)) == (COMPOSITE, [0, 0, 0, 0])
    r = fpng_amd.view_alpha("composite", (255, np.uint8(7), 1))
    assert (r.op, list(r.background), list(r.reserved)) == (COMPOSITE, [255, 7, 1, 0], [0, 0])
    r = fpng_amd.view_alpha(op="premultiplied")
    assert (r.op, list(r.background)) == (PREMULTIPLIED, [0, 0, 0, 0])
    for bad in (lambda: fpng_amd.view_alpha("over"), lambda: fpng_amd.view_alpha(1), lambda: fpng_amd.view_alpha("composite", (1, 2)), lambda: fpng_amd.view_alpha("composite", (1, 2, 3, 4)),
                lambda: fpng_amd.view_alpha("composite", (1, 2, 256)), lambda: fpng_amd.view_alpha("composite", (-1, 2, 3)), lambda: fpng_amd.view_alpha("composite", (0.5, 2, 3)),
                lambda: fpng_amd.view_alpha("composite", 255), lambda: fpng_amd.view_alpha("premultiplied", (1, 0, 0)), lambda: fpng_amd.view_alpha(None, (0, 0, 1)),
                lambda: fpng_amd.view_alpha_source({"op": "composite"}, np.zeros((4, 2, 2), dtype=np.uint8)), lambda: fpng_amd.view_alpha_source(r, np.zeros((3, 2, 2), dtype=np.uint8)),
                lambda: fpng_amd.view_alpha_result(r, np.zeros((4, 2, 2), dtype=np.float32)), lambda: fpng_amd.view_alpha_result(r, np.zeros((4, 0, 2), dtype=np.uint8)),
                lambda: fpng_amd.view_alpha_result(fpng_amd.view_tone(), np.zeros((4, 2, 2), dtype=np.uint8))):
        with pytest.raises(ValueError):
            bad()


@pytest.mark.parametrize("hwc", [False, True])
def test_the_alpha_keyword_shapes_and_lengths(hwc):
    """make_decode_batch_views(_hwc)(..., alpha=) needs no GPU: one record, one per file, one per view; wrong lengths and types raise;
    without alpha= the descriptor goes where it went"""
    from fpng_amd.api import views_entry
    make = Encoder.make_decode_batch_views_hwc if hwc else Encoder.make_decode_batch_views
    layout = "hwc" if hwc else "planar"
    pngs = [b"x" * 8, b"y" * 8]
    crops = [[(0, 0, 8, 8), (1, 1, 4, 4)], [(0, 0, 8, 8)]]
    outs = [[torch.empty((4, 4, 3) if hwc else (3, 4, 4), dtype=torch.uint8) for _ in cs] for cs in crops]
    a, b = fpng_amd.view_alpha("composite", (255, 255, 255)), fpng_amd.view_alpha("premultiplied")
    db = make(pngs, crops, outs, (4, 4), enhance=fpng_amd.view_enhance(color=0.5))
    assert db.alphas is None and views_entry(layout, False, db)[0] == f"fpng_amd_decode_batch_{layout}_views_enhance"
    assert views_entry(layout, False, make(pngs, crops, outs, (4, 4)))[0] == f"fpng_amd_decode_batch_{layout}_views"
    db = make(pngs, crops, outs, (4, 4), alpha=a)
    assert db.colors is None and db.posts is None and db.warps is None and db.tones is None and db.enhances is None
    assert [(p.op, list(p.background)) for p in db.alphas] == [(COMPOSITE, [255, 255, 255, 0])] * 3
    symbol, args = views_entry(layout, False, db)
    assert symbol == f"fpng_amd_decode_batch_{layout}_views_alpha" and args[6:11] == [None] * 5 and args[11] is db.alphas and len(args) == 14
    db = make(pngs, crops, outs, (4, 4), alpha=[a, b])
    assert [p.op for p in db.alphas] == [COMPOSITE, COMPOSITE, PREMULTIPLIED]
    db = make(pngs, crops, outs, (4, 4), alpha=[[b, a], [fpng_amd.view_alpha()]], color=np.eye(3, 4), tone=fpng_amd.view_tone(equalize=True))
    assert db.colors is not None and db.tones is not None and db.posts is None and [p.op for p in db.alphas] == [PREMULTIPLIED, COMPOSITE, 0]
    for bad in ([a], [a, b, a], [[a], [b]], [[a, b, a], b], [[a, b], []], 3, [a, 3], [[a, {"op": "composite"}], b], "ab", fpng_amd.view_post(), fpng_amd.view_enhance()):
        with pytest.raises(ValueError):
            make(pngs, crops, outs, (4, 4), alpha=bad)


# ---- 4. what the plan makes of the records ----
def test_the_view_plan_carries_the_records(built_lib, tmp_path):
    """tests/cpp/view_plan_alpha.cpp, a stand-alone program over view_plan.h, run on the CPU: the op and background travel in the
    resize record's flags next to the mirror flag and leave the record's other fields alone; a record of a 3-channel file normalises
    to op 0; the job of a 4-channel file with an alpha view decodes four planes into the scratch, whatever the destination has, and
    no other job does; a plan without alpha records is the plan that it was"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "view_plan_alpha")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cmd = ["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(root, "fpng_amd", "csrc"),
           "-I", os.path.join(root, "include"), "-I", os.path.join(rocm, "include"), os.path.join(root, "tests", "cpp", "view_plan_alpha.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and not run.stderr, (run.returncode, run.stdout[-2000:], run.stderr[-2000:])
    assert run.stdout.splitlines() == ["ok planar", "ok hwc"]


# ---- 5. the conditions on the GPU test's images ----
def test_the_pattern_meets_the_conditions():
    """the pattern under a bicubic upscale has samples where U's clip is live, samples with R'_3 == 0 under a colour that is not 0,
    and source alpha of 0, of 255 and in between; under bilinear the weights are not negative and the first two never occur"""
    for (w, h), full in (((33, 9), (70, 20)), ((90, 40), (200, 90))):
        px4 = _planes(AM.pattern(w, h))
        got = AM.conditions(px4, full, "bicubic")
        assert all(got[k] >= 1 for k in ("clip", "zero_alpha_colour", "alpha_0", "alpha_255", "alpha_between")), got
        lin = AM.conditions(px4, full, "bilinear")
        assert lin["clip"] == 0 and lin["zero_alpha_colour"] == 0, lin
    # (bright where opaque)
    px = AM.pattern(90, 40)
    assert (px[..., :3][px[..., 3] == 255] >= 200).all()
