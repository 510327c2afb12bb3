"""No-GPU tests of the per-view affine warp of the views calls (fpng_amd_decode_batch(_device)_planar_views_warp /
_hwc_views_warp): the exact model of warp_model.py and the host twin fpng_amd_view_warp_apply -- the text the kernel runs -- against
Pillow's Image.transform(size, AFFINE, a, resample, fillcolor), whole images bit for bit, for the classes of matrices the rule
is Pillow's for; the twin against the model everywhere, mirrored and not; affine_matrix by its properties; every call-level refusal,
none of which needs an encoder or a device; the Python door."""
import ctypes as C
import math

import numpy as np
import pytest
import torch
from PIL import Image

import fpng_amd
from fpng_amd import _lib
from fpng_amd.api import Encoder

import warp_model as WM
from test_resize_view_cpu import GOOD
from test_views_post_cpu import _arrays, _fill as _fill_post

PLANAR = ("fpng_amd_decode_batch_planar_views_warp", "fpng_amd_decode_batch_device_planar_views_warp")
HWC = ("fpng_amd_decode_batch_hwc_views_warp", "fpng_amd_decode_batch_device_hwc_views_warp")
WIDTHS, HEIGHTS = (1, 2, 3, 17, 64, 65, 130), (1, 2, 16, 17, 33)
SIZES = [(w, h) for w in WIDTHS for h in HEIGHTS]
FILTERS = {"nearest": Image.NEAREST, "bilinear": Image.BILINEAR}
FILLS = [(0, 0, 0), (255, 255, 255), (7, 128, 250), (1, 2, 3)]


def _image(w, h, seed):
    """(h, w, 3) bytes: noise, a gradient along x and one along y"""
    rng = np.random.default_rng(seed)
    gx = np.broadcast_to(np.rint(np.linspace(0, 255, w)).astype(np.uint8)[None, :], (h, w))
    gy = np.broadcast_to(np.rint(np.linspace(255, 0, h)).astype(np.uint8)[:, None], (h, w))
    return np.ascontiguousarray(np.stack([rng.integers(0, 256, size=(h, w), dtype=np.uint8), gx, gy], axis=-1))


def _pillow(img, a, filter, fill):
    h, w = img.shape[:2]
    return np.asarray(Image.fromarray(img).transform((w, h), Image.AFFINE, tuple(a), FILTERS[filter], fillcolor=tuple(fill)))


def _general(rng, w, h):
    """rotation within +-45 degrees x scale 0.7 .. 1.4 x shear x a fractional translation, about the centre (a1 != 0 or a3 != 0)"""
    while True:
        a = fpng_amd.affine_matrix(w, h, angle=rng.uniform(-45, 45), translate=(rng.uniform(-0.4, 0.4) * w, rng.uniform(-0.4, 0.4) * h), scale=rng.uniform(0.7, 1.4),
                                   shear=(rng.uniform(-20, 20), rng.uniform(-20, 20)))
        if a[1] != 0.0 or a[3] != 0.0:
            return a


def _shear(rng, w, h):
    """a pure shear along x or along y, with its translation"""
    s, t = rng.uniform(-0.9, 0.9), rng.uniform(-3, 3)
    return [1.0, s, t, 0.0, 1.0, 0.0] if rng.integers(2) else [1.0, 0.0, 0.0, s, 1.0, t]


def _translation(rng, w, h):
    """a pure translation by integers or half-integers, some of them wholly outside"""
    tx, ty = (int(rng.integers(-2 * (n + 1), 2 * (n + 1) + 1)) * 0.5 for n in (w, h))
    return [1.0, 0.0, tx, 0.0, 1.0, ty]


def _cases():
    """(w, h, a, filter, fill, seed): every size, 12 matrices each -- 420 in all, a third of each class, both filters, every fill"""
    rng = np.random.default_rng(20240607)
    out = []
    for n, (w, h) in enumerate(SIZES):
        for k in range(12):
            a = (_general, _shear, _translation)[k % 3](rng, w, h)
            out.append((w, h, a, ("nearest", "bilinear")[(k // 3 + n) % 2], FILLS[(k + n) % len(FILLS)], 1000 * n + k))
    return out


CASES = _cases()


def _record(a, filter, fill):
    return fpng_amd.view_warp(a, filter, fill)


def _twin(a, filter, fill, img, mirror):
    """the host twin on the three planes of img (B: un-mirrored), each with its own fill"""
    rec = _record(a, filter, fill)
    return np.stack([fpng_amd.view_warp_apply(rec, img[..., k], mirror, fill[k]) for k in range(3)], axis=-1)


def _model(a, filter, fill, img, mirror):
    warp = {"a": a, "filter": filter, "fill": list(fill) + [255]}
    return np.stack([WM.apply_plane(warp, img[..., k], mirror, fill[k]) for k in range(3)], axis=-1)


def test_entry_points_and_record(built_lib):
    lib = _lib.load()
    for name in PLANAR + HWC + ("fpng_amd_view_warp_apply",):
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
    assert lib.fpng_amd_abi_version() == 5  # (new entry points, the same ABI version)
    assert C.sizeof(_lib.ViewWarp) == 64
    assert {n: getattr(_lib.ViewWarp, n).offset for n, _ in _lib.ViewWarp._fields_} == {"flags": 0, "reserved0": 4, "a": 8, "fill": 56, "reserved1": 60}
    assert (_lib.WARP_AFFINE, _lib.WARP_BILINEAR) == (1, 2)


# ---- against Pillow ----
def test_the_model_and_the_host_twin_are_pillows(built_lib):
    """420 seeded matrices over every size: rotation x scale x shear x fractional translation, pure shears, integer and
    half-integer translations; both filters, four fills.  Whole images equal, the model's and the twin's; mirrored: Pillow on the
    flipped image"""
    assert len(CASES) >= 300 and {c[3] for c in CASES} == set(FILTERS)
    for w, h, a, filter, fill, seed in CASES:
        assert WM.corners_ok(a, w, h)
        img = _image(w, h, seed)
        for mirror in (False, True):
            want = _pillow(np.ascontiguousarray(img[:, ::-1]) if mirror else img, a, filter, fill)
            model, twin = _model(a, filter, fill, img, mirror), _twin(a, filter, fill, img, mirror)
            assert np.array_equal(model, want), ("model", w, h, a, filter, fill, mirror, int(np.count_nonzero(model != want)))
            assert np.array_equal(twin, want), ("twin", w, h, a, filter, fill, mirror, int(np.count_nonzero(twin != want)))


def test_fractional_pure_scale_nearest_keeps_the_fixed_point_rule(built_lib):
    """a1 == a3 == 0 with a fractional scale, nearest: Pillow's own path there runs on double sums and may differ in rare ties.  The
    twin is the model on every matrix; the share of matrices on which the model is not Pillow's is printed, and capped at 2 % as a
    guard against a wrong model (it is no tolerance on the library)"""
    rng = np.random.default_rng(77)
    differ, total = 0, 0
    for n in range(400):
        w, h = SIZES[n % len(SIZES)]
        a = [rng.uniform(0.6, 1.6), 0.0, rng.uniform(-3, 3), 0.0, rng.uniform(0.6, 1.6), rng.uniform(-3, 3)]
        img, fill = _image(w, h, n), FILLS[n % len(FILLS)]
        for mirror in (False, True):
            assert np.array_equal(_twin(a, "nearest", fill, img, mirror), _model(a, "nearest", fill, img, mirror)), (w, h, a, mirror)
        differ += not np.array_equal(_model(a, "nearest", fill, img, False), _pillow(img, a, "nearest", fill))
        total += 1
    print(f"fractional pure-scale nearest: the model differs from Pillow on {differ} of {total} matrices")
    assert differ <= 0.02 * total, (differ, total)


def test_bilinear_pure_scale_is_pillows(built_lib):
    """the bilinear rule has one path: fractional pure scale / translate matrices too"""
    rng = np.random.default_rng(78)
    for n in range(70):
        w, h = SIZES[n % len(SIZES)]
        a = [rng.uniform(0.6, 1.6), 0.0, rng.uniform(-3, 3), 0.0, rng.uniform(0.6, 1.6), rng.uniform(-3, 3)]
        img, fill = _image(w, h, n), FILLS[n % len(FILLS)]
        want = _pillow(img, a, "bilinear", fill)
        assert np.array_equal(_model(a, "bilinear", fill, img, False), want) and np.array_equal(_twin(a, "bilinear", fill, img, False), want), (w, h, a)


@pytest.mark.parametrize("filter", list(FILTERS))
def test_the_identity_is_the_input(built_lib, filter):
    for n, (w, h) in enumerate(SIZES):
        img = _image(w, h, n)
        for a in (WM.IDENTITY, fpng_amd.affine_matrix(w, h)):
            assert np.array_equal(_twin(a, filter, (9, 9, 9), img, False), img) and np.array_equal(_model(a, filter, (9, 9, 9), img, False), img), (w, h, a)
            assert np.array_equal(_twin(a, filter, (9, 9, 9), img, True), img[:, ::-1]), (w, h, a)
    none = fpng_amd.view_warp()  # (a record without flags: the mirrored window)
    assert np.array_equal(fpng_amd.view_warp_apply(none, img[..., 0], True), img[:, ::-1, 0]) and np.array_equal(WM.apply_plane({}, img[..., 0], True), img[:, ::-1, 0])


# ---- affine_matrix ----
def test_affine_matrix_by_its_properties(built_lib):
    assert [abs(v) for v in fpng_amd.affine_matrix(65, 17)] == [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]
    for n in (2, 16, 64):  # a quarter turn of an even square
        img = _image(n, n, n)
        a = fpng_amd.affine_matrix(n, n, angle=90)
        assert np.array_equal(_twin(a, "nearest", (5, 5, 5), img, False), np.rot90(img, k=-1)), n
        # (cos(pi / 2) is 6e-17 in doubles, not 0: a bilinear position lies that far off a sample, and the blend, TRUNCATED as Pillow
        #  truncates it, may be one below the sample -- never more, and never fill)
        lin = _twin(a, "bilinear", (5, 5, 5), img, False)
        assert np.array_equal(lin, _pillow(img, a, "bilinear", (5, 5, 5))) and np.abs(lin.astype(int) - np.rot90(img, k=-1)).max() <= 1, n
    img = _image(65, 17, 3)
    for tx, ty in ((3, 0), (0, -2), (-7, 5), (65, 0), (0, 17), (-64, -16)):  # a shift with fill
        want = np.empty_like(img)
        want[...] = (7, 128, 250)
        ys, xs = slice(max(ty, 0), 17 + min(ty, 0)), slice(max(tx, 0), 65 + min(tx, 0))
        want[ys, xs] = img[slice(max(-ty, 0), 17 + min(-ty, 0)), slice(max(-tx, 0), 65 + min(-tx, 0))]
        a = fpng_amd.affine_matrix(65, 17, translate=(tx, ty))
        for filter in FILTERS:
            assert np.array_equal(_twin(a, filter, (7, 128, 250), img, False), want), (tx, ty, filter)
            assert np.array_equal(_pillow(img, a, filter, (7, 128, 250)), want), (tx, ty, filter)
    # scale and shear: the inverse map of the forward matrix about the centre, by its definition
    w, h, angle, scale, sx, sy, tx, ty = 40, 30, 25.0, 1.3, 10.0, -5.0, 3.0, -2.0
    a = fpng_amd.affine_matrix(w, h, angle=angle, translate=(tx, ty), scale=scale, shear=(sx, sy))
    rot, kx, ky = math.radians(angle), math.radians(sx), math.radians(sy)
    rss = scale * np.array([[math.cos(rot - ky) / math.cos(ky), -math.cos(rot - ky) * math.tan(kx) / math.cos(ky) - math.sin(rot)],
                            [math.sin(rot - ky) / math.cos(ky), -math.sin(rot - ky) * math.tan(kx) / math.cos(ky) + math.cos(rot)]])
    inv = np.linalg.inv(rss)
    centre = np.array([w * 0.5, h * 0.5])
    for p in ((0.0, 0.0), (12.5, 7.25), (40.0, 30.0)):
        want = inv @ (np.array(p) - centre - (tx, ty)) + centre
        got = (a[0] * p[0] + a[1] * p[1] + a[2], a[3] * p[0] + a[4] * p[1] + a[5])
        assert np.allclose(got, want, rtol=0, atol=1e-9), (p, got, want)
    assert fpng_amd.affine_matrix(10, 10, center=(0, 0), angle=30)[2] == 0.0
    for bad in ({"scale": 0}, {"shear": (1, 2, 3)}, {"translate": 3}):
        with pytest.raises((ValueError, TypeError)):
            fpng_amd.affine_matrix(8, 8, **bad)


# ---- refusals ----
AFFINE, BILINEAR = _lib.WARP_AFFINE, _lib.WARP_BILINEAR
NAN, INF = float("nan"), float("inf")
IDENT = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
# (flags, reserved0, a, fill, reserved1) and a piece of the message; the record's view is GOOD[1]: a 6 x 4 window
BAD_RECORDS = [((4, 0, IDENT, (0, 0, 0, 0), 0), "unknown fpng_amd_view_warp::flags"), ((0x80000000 | AFFINE, 0, IDENT, (0, 0, 0, 0), 0), "unknown fpng_amd_view_warp::flags"),
               ((BILINEAR, 0, IDENT, (0, 0, 0, 0), 0), "FPNG_AMD_WARP_BILINEAR needs FPNG_AMD_WARP_AFFINE"),
               ((AFFINE, 1, IDENT, (0, 0, 0, 0), 0), "reserved0 and reserved1 must be 0"), ((0, 0, (0.0,) * 6, (0, 0, 0, 0), 9), "reserved0 and reserved1 must be 0"),
               ((AFFINE, 0, (NAN, 0.0, 0.0, 0.0, 1.0, 0.0), (0, 0, 0, 0), 0), "must be finite"), ((AFFINE | BILINEAR, 0, (1.0, 0.0, 0.0, 0.0, 1.0, INF), (0, 0, 0, 0), 0), "must be finite"),
               ((AFFINE, 0, (1.0, 0.0, -INF, 0.0, 1.0, 0.0), (0, 0, 0, 0), 0), "must be finite"), ((0, 0, (0.0, 0.0, 0.0, NAN, 0.0, 0.0), (0, 0, 0, 0), 0), "must be finite"),
               ((AFFINE, 0, (1.0, 0.0, 32768.0, 0.0, 1.0, 0.0), (0, 0, 0, 0), 0), "check_fixed"), ((AFFINE | BILINEAR, 0, (1.0, 0.0, 0.0, 0.0, 1.0, -32768.0), (0, 0, 0, 0), 0), "check_fixed"),
               ((AFFINE, 0, (1.0, 0.0, 32762.0, 0.0, 1.0, 0.0), (0, 0, 0, 0), 0), "check_fixed"),  # (corner (w, 0): 32762 + 6)
               ((AFFINE | BILINEAR, 0, (1.0, 0.0, 0.0, 0.0, 1.0, 32764.0), (0, 0, 0, 0), 0), "check_fixed"),  # (corner (0, h): 32764 + 4)
               ((AFFINE, 0, (1.0, 0.0, 0.0, 7000.0, 7000.0, -30000.0), (0, 0, 0, 0), 0), "check_fixed"),  # (corner (w, h) alone: 42000 + 28000 - 30000)
               ((0, 0, IDENT, (0, 0, 0, 0), 0), "must be 0 without FPNG_AMD_WARP_AFFINE"), ((0, 0, (0.0,) * 5 + (1e-300,), (0, 0, 0, 0), 0), "must be 0 without FPNG_AMD_WARP_AFFINE"),
               ((0, 0, (0.0,) * 6, (0, 0, 0, 1), 0), "must be 0 without FPNG_AMD_WARP_AFFINE")]
GOOD_RECORDS = [(0, 0, (0.0,) * 6, (0, 0, 0, 0), 0), (0, 0, (-0.0,) * 6, (0, 0, 0, 0), 0), (AFFINE, 0, IDENT, (1, 2, 3, 4), 0), (AFFINE | BILINEAR, 0, IDENT, (255, 0, 0, 255), 0),
                (AFFINE, 0, (1.0, 0.0, 32761.0, 0.0, 1.0, -32767.0), (0, 0, 0, 0), 0), (AFFINE | BILINEAR, 0, (0.0,) * 6, (0, 0, 0, 0), 0),
                (AFFINE, 0, (-5000.0, 0.0, 100.0, 0.0, 8000.0, -3.0), (0, 0, 0, 0), 0)]


def _fill(rec, values):
    rec.flags, rec.reserved0, rec.reserved1 = values[0], values[1], values[4]
    for k in range(6):
        rec.a[k] = values[2][k]
    for k in range(4):
        rec.fill[k] = values[3][k]


@pytest.mark.parametrize("name", PLANAR + HWC)
def test_call_level_refusals_need_no_encoder(built_lib, name):
    """with a NULL encoder every call returns -1 and the message names the reason: a bad argument its own, a good set only the
    missing encoder"""
    lib = _lib.load()
    fn, hwc = getattr(lib, name), name in HWC
    fmt = _lib.FloatFormat()

    def why():
        return lib.fpng_amd_last_error().decode()

    def fresh():  # the second record's window is 6 x 4
        files, cnt, c, v, d, col, post, res = _arrays([GOOD[0], GOOD[1], GOOD[2]], [2, 1], hwc)
        return files, cnt, c, v, d, col, post, (_lib.ViewWarp * 3)(), res

    files, cnt, c, v, d, col, post, warp, res = fresh()
    for colors, posts in ((col, post), (None, post), (col, None), (None, None)):  # (NULL colors: the identity; NULL posts: no post flags)
        assert fn(None, files, 2, cnt, c, v, d, colors, posts, warp, None, res) == -1 and "null/empty batch" in why(), why()  # (nothing is at fault -- the batch has no encoder)
        assert fn(None, files, 2, cnt, c, v, d, colors, posts, warp, C.byref(fmt), res) == -1 and "null/empty batch" in why(), why()
        assert fn(None, files, 2, cnt, c, v, d, colors, posts, None, None, res) == -1 and "null warps" in why(), why()
    # ---- the records ----
    for posts in (True, False):
        for values, piece in BAD_RECORDS:
            files, cnt, c, v, d, col, post, warp, res = fresh()
            _fill(warp[1], values)
            assert fn(None, files, 2, cnt, c, v, d, col, post if posts else None, warp, None, res) == -1 and piece in why(), (values, why())
        for values in GOOD_RECORDS:
            files, cnt, c, v, d, col, post, warp, res = fresh()
            _fill(warp[1], values)
            assert fn(None, files, 2, cnt, c, v, d, col, post if posts else None, warp, None, res) == -1 and "null/empty batch" in why(), (values, why())
    # (the corners are the record's own window's: 32763.5 passes 3 x 2 and 1 x 1, not 6 x 4; the last record of the call is judged too)
    for at, ok in ((0, True), (1, False), (2, True)):
        files, cnt, c, v, d, col, post, warp, res = fresh()
        _fill(warp[at], (AFFINE, 0, (1.0, 0.0, 32763.5, 0.0, 1.0, 0.0), (0, 0, 0, 0), 0))
        assert fn(None, files, 2, cnt, c, v, d, col, post, warp, None, res) == -1 and ("null/empty batch" if ok else "check_fixed") in why(), (at, why())
    files, cnt, c, v, d, col, post, warp, res = fresh()
    _fill(warp[2], BAD_RECORDS[0][0])
    assert fn(None, files, 2, cnt, c, v, d, col, post, warp, None, res) == -1 and "fpng_amd_view_warp::flags" in why(), why()
    # ---- everything the post call refuses ----
    files, cnt, c, v, d, col, post, warp, res = fresh()
    _fill(warp[0], GOOD_RECORDS[2])
    _fill_post(post[1], (_lib.POST_BLUR, 4, 1.0, 0, 0, (0, 0)))
    assert fn(None, files, 2, cnt, c, v, d, col, post, warp, None, res) == -1 and "below the window" in why(), why()  # (the blur's R < min(w, h) is unchanged)
    _fill_post(post[1], (_lib.POST_SOLARIZE, 0, 0.0, 256, 0, (0, 0)))
    assert fn(None, files, 2, cnt, c, v, d, col, post, warp, None, res) == -1 and "solarize_threshold" in why(), why()
    _fill_post(post[1], (_lib.POST_BLUR, 3, 1.0, 0, 0, (0, 0)))
    col[2].m[1][1] = float("nan")
    assert fn(None, files, 2, cnt, c, v, d, col, post, warp, None, res) == -1 and "fpng_amd_view_color::m" in why(), why()
    col[2].m[1][1] = 1.0
    good = [files, 2, cnt, c, v, d, col, post, warp, None, res]
    assert fn(None, *good) == -1 and "null/empty batch" in why(), why()
    for k in (0, 2, 3, 4, 5, 10):  # a null array
        args = list(good)
        args[k] = None
        assert fn(None, *args) == -1 and "null files, view_count, crops, views, dests or results" in why(), (k, why())
    for counts in ([0, 3], [3, 0]):
        assert fn(None, files, 2, (C.c_uint32 * 2)(*counts), c, v, d, col, post, warp, None, res) == -1 and "view_count of 0" in why(), (counts, why())
    v[1].filter = 2
    assert fn(None, *good) == -1 and "filter" in why(), why()
    v[1].filter = 1
    files[1].row_pitch = 4
    assert fn(None, *good) == -1 and "must be NULL / 0" in why(), why()


def test_the_host_twin_refuses_what_the_calls_refuse(built_lib):
    lib = _lib.load()
    plane = np.zeros((4, 6), dtype=np.uint8)
    out = np.zeros_like(plane)
    for values, piece in BAD_RECORDS:
        rec = _lib.ViewWarp()
        _fill(rec, values)
        with pytest.raises(fpng_amd.FpngAmdError, match=piece.replace("(", r"\(").replace(")", r"\)")):
            fpng_amd.view_warp_apply(rec, plane)
    for values in GOOD_RECORDS:
        rec = _lib.ViewWarp()
        _fill(rec, values)
        fpng_amd.view_warp_apply(rec, plane)
    rec = fpng_amd.view_warp(IDENT)
    assert lib.fpng_amd_view_warp_apply(None, 6, 4, 0, plane.ctypes.data, out.ctypes.data, 0) == -1
    assert lib.fpng_amd_view_warp_apply(C.byref(rec), 6, 4, 0, None, out.ctypes.data, 0) == -1
    assert lib.fpng_amd_view_warp_apply(C.byref(rec), 6, 4, 0, plane.ctypes.data, None, 0) == -1
    assert lib.fpng_amd_view_warp_apply(C.byref(rec), 0, 4, 0, plane.ctypes.data, out.ctypes.data, 0) == -1
    assert lib.fpng_amd_view_warp_apply(C.byref(rec), 6, 0, 0, plane.ctypes.data, out.ctypes.data, 0) == -1


# ---- the Python door ----
def test_view_warp():
    r = fpng_amd.view_warp()
    assert (r.flags, r.reserved0, list(r.a), list(r.fill), r.reserved1) == (0, 0, [0.0] * 6, [0, 0, 0, 0], 0)
    r = fpng_amd.view_warp([1, 0.5, -3, 0, 1, 2.25])
    assert (r.flags, list(r.a), list(r.fill)) == (1, [1.0, 0.5, -3.0, 0.0, 1.0, 2.25], [0, 0, 0, 0])
    r = fpng_amd.view_warp(np.arange(6), "bilinear", 128)
    assert (r.flags, list(r.a), list(r.fill)) == (3, [0.0, 1.0, 2.0, 3.0, 4.0, 5.0], [128, 128, 128, 128])
    assert list(fpng_amd.view_warp(IDENT, fill=(1, 2, 3)).fill) == [1, 2, 3, 255] and list(fpng_amd.view_warp(IDENT, fill=(1, 2, 3, 4)).fill) == [1, 2, 3, 4]
    for bad in ({"matrix": [1, 0, 0]}, {"matrix": 3}, {"matrix": "abcdef"}, {"matrix": IDENT, "filter": "bicubic"}, {"matrix": IDENT, "fill": 256},
                {"matrix": IDENT, "fill": -1}, {"matrix": IDENT, "fill": 1.5}, {"matrix": IDENT, "fill": (1, 2, 3, 4, 5)}, {"matrix": IDENT, "fill": ()}):
        with pytest.raises(ValueError):
            fpng_amd.view_warp(**bad)
    with pytest.raises(ValueError):
        fpng_amd.view_warp_apply({"a": IDENT}, np.zeros((2, 2), dtype=np.uint8))
    with pytest.raises(ValueError):
        fpng_amd.view_warp_apply(r, np.zeros((2, 2, 3), dtype=np.uint8))


@pytest.mark.parametrize("hwc", [False, True])
def test_the_warp_keyword_shapes_and_lengths(hwc):
    """make_decode_batch_views(_hwc)(..., warp=) needs no GPU: one record, one per file, one per view; wrong lengths and types raise"""
    make = Encoder.make_decode_batch_views_hwc if hwc else Encoder.make_decode_batch_views
    pngs = [b"x" * 8, b"y" * 8]
    crops = [[(0, 0, 8, 8), (1, 1, 4, 4)], [(0, 0, 8, 8)]]
    outs = [[torch.empty((4, 4, 3) if hwc else (3, 4, 4), dtype=torch.uint8) for _ in cs] for cs in crops]
    a, b = fpng_amd.view_warp(IDENT), fpng_amd.view_warp(IDENT, "bilinear", 3)
    assert make(pngs, crops, outs, (4, 4)).warps is None and make(pngs, crops, outs, (4, 4), post=fpng_amd.view_post(solarize=1)).warps is None
    db = make(pngs, crops, outs, (4, 4), warp=a)
    assert db.colors is None and db.posts is None and [(p.flags, p.fill[3]) for p in db.warps] == [(1, 0)] * 3
    db = make(pngs, crops, outs, (4, 4), warp=[a, b])
    assert [p.flags for p in db.warps] == [1, 1, 3]
    db = make(pngs, crops, outs, (4, 4), warp=[[b, a], [fpng_amd.view_warp()]], color=np.eye(3, 4), post=fpng_amd.view_post(posterize=2))
    assert db.colors is not None and db.posts is not None and [p.flags for p in db.warps] == [3, 1, 0]
    for bad in ([a], [a, b, a], [[a], [b]], [[a, b, a], b], [[a, b], []], 3, [a, 3], [[a, {"a": IDENT}], b], "ab", fpng_amd.view_post()):
        with pytest.raises(ValueError):
            make(pngs, crops, outs, (4, 4), warp=bad)


# ---- the host twin under the sanitizers ----
def _sanitizer_cases():
    """(w, h, mirror, flags, fill, a): every edge shape under both filters, mirrored and not -- rotations that leave fill in the corners,
    shears, translations wholly outside, positions at the limit of the corner check, a 1-sample axis whose coefficient does not fit
    16.16 in 32 bits; and records the calls refuse"""
    out = []
    for n, (w, h) in enumerate(SIZES):
        ms = [list(IDENT), fpng_amd.affine_matrix(w, h, angle=30.0 + n), fpng_amd.affine_matrix(w, h, angle=-45.0, scale=0.75, shear=(10.0, -5.0)), [1.0, 0.0, 0.5, 0.0, 1.0, -0.5],
              [1.0, 0.8, -1.5, 0.0, 1.0, 0.0], [1.0, 0.0, float(-w), 0.0, 1.0, 0.0], [1.0, 0.0, 0.0, 0.0, 1.0, float(h)], [1.0, 0.0, 32767.0 - w, 0.0, 1.0, -32767.0],
              [-1.0, 0.0, float(w), 0.0, -1.0, float(h)], [32000.0 / w, 0.0, 0.0, 0.0, -32000.0 / h, 32000.0], [0.0, 0.0, w * 0.5, 0.0, 0.0, h * 0.5]]
        for k, a in enumerate(ms):
            out.append((w, h, (n + k) & 1, 1 + 2 * ((n + k) >> 1 & 1), (37 * n + k) & 255, a))
            out.append((w, h, (n + k + 1) & 1, 3 - 2 * ((n + k) >> 1 & 1), (91 * n + k) & 255, a))
        out.append((w, h, n & 1, 0, 0, [0.0] * 6))
    out += [(6, 4, 0, 2, 0, list(IDENT)), (6, 4, 0, 1, 0, [1.0, 0.0, 32768.0, 0.0, 1.0, 0.0]), (6, 4, 1, 3, 0, [NAN, 0.0, 0.0, 0.0, 1.0, 0.0]), (6, 4, 0, 0, 0, list(IDENT))]
    return out


def test_the_host_twin_under_the_sanitizers(built_lib, tmp_path):
    """tests/cpp/view_warp_apply.cpp, a stand-alone program over view_warp.h built with the address and undefined-behaviour
    sanitizers and run on the CPU: no report, and every plane it prints is the model's"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "view_warp_apply")
    # (-Wno-unknown-pragmas: the header's `#pragma clang fp contract`; g++ in ISO mode does not contract on x86-64.  The sanitizers'
    #  runtimes are linked into the program where the compiler has them as archives, so that it starts in any environment)
    cmd = ["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-I", os.path.join(root, "fpng_amd", "csrc"),
           "-I", os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "view_warp_apply.cpp"), "-o", exe]
    r = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if r.returncode != 0:
        r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    cases = _sanitizer_cases()
    text = "".join("%d %d %d %d %d %s\n" % (w, h, mirror, flags, fill, " ".join(float(v).hex() for v in a)) for w, h, mirror, flags, fill, a in cases)
    env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([exe], input=text, capture_output=True, text=True, env=env, timeout=120)
    assert run.returncode == 0 and not run.stderr, (run.returncode, run.stderr[-2000:])
    lines = run.stdout.splitlines()
    assert len(lines) == len(cases)
    refused = 0
    for (w, h, mirror, flags, fill, a), ln in zip(cases, lines):
        x, y = np.arange(w, dtype=np.int64)[None, :], np.arange(h, dtype=np.int64)[:, None]
        plane = ((7 * x + 13 * y + x * y) & 255).astype(np.uint8)
        ok = flags in (0, 1, 3) and all(math.isfinite(v) for v in a) and (WM.corners_ok(a, w, h) if flags else not any(a))
        if not ok:
            assert ln.startswith("refused "), (w, h, flags, a, ln[:80])
            refused += 1
            continue
        want = WM.apply_plane({"a": a, "filter": "bilinear" if flags & 2 else "nearest", "fill": [fill] * 4} if flags else {}, plane, bool(mirror), fill)
        assert ln == "ok " + want.tobytes().hex(), (w, h, mirror, flags, fill, a)
    assert refused == 4
