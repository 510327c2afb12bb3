"""No-GPU tests of the per-view post-processing of the views calls (fpng_amd_decode_batch(_device)_planar_views_post /
_hwc_views_post: Gaussian blur, solarize, posterize): the host's weights and the host twin fpng_amd_view_post_apply -- the text the
kernel runs -- against the exact model of post_model.py, bit for bit; the point operations against Pillow; the blur against an
independent double-precision one (scipy); every call-level refusal, none of which needs an encoder or a device; the Python door."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import fpng_amd
from fpng_amd import _lib
from fpng_amd.api import Encoder

import post_model as PM
from test_resize_view_cpu import GOOD

PLANAR = ("fpng_amd_decode_batch_planar_views_post", "fpng_amd_decode_batch_device_planar_views_post")
HWC = ("fpng_amd_decode_batch_hwc_views_post", "fpng_amd_decode_batch_device_hwc_views_post")
RADII, SIGMAS = (1, 2, 11, 16), (0.1, 0.5, 1.3, 2.0, 5.0)
# (w, h) and the radii each plane is blurred with: 17 x 17 at R = 16 reflects to the far edge from both sides
SHAPES = [((17, 17), (16,)), ((129, 33), (16, 11, 1)), ((64, 97), (16, 2)), ((2, 2), (1,))]


def _record(post):
    return fpng_amd.view_post(blur=(2 * post["blur"][0] + 1, post["blur"][1]) if "blur" in post else None, solarize=post.get("solarize"), posterize=post.get("posterize"))


def _planes(w, h, seed):
    """a noise plane and two gradients (one per axis, the full range) of w x h bytes"""
    rng = np.random.default_rng(seed)
    gx = np.broadcast_to(np.rint(np.linspace(0, 255, w)).astype(np.uint8)[None, :], (h, w))
    gy = np.broadcast_to(np.rint(np.linspace(255, 0, h)).astype(np.uint8)[:, None], (h, w))
    return {"noise": rng.integers(0, 256, size=(h, w), dtype=np.uint8), "gradient_x": np.ascontiguousarray(gx), "gradient_y": np.ascontiguousarray(gy)}


def test_entry_points_and_record(built_lib):
    lib = _lib.load()
    for name in PLANAR + HWC + ("fpng_amd_blur_weights", "fpng_amd_view_post_apply"):
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
    assert lib.fpng_amd_abi_version() == 5  # (new entry points, the same ABI version)
    assert C.sizeof(_lib.ViewPost) == 32
    assert {n: getattr(_lib.ViewPost, n).offset for n, _ in _lib.ViewPost._fields_} == {"flags": 0, "blur_radius": 4, "blur_sigma": 8, "solarize_threshold": 16,
                                                                                       "posterize_bits": 20, "reserved": 24}


# ---- the weights ----
@pytest.mark.parametrize("sigma", SIGMAS)
@pytest.mark.parametrize("radius", RADII)
def test_the_weights_are_the_models(built_lib, radius, sigma):
    want = PM.blur_weights(radius, sigma)
    got = fpng_amd.blur_weights(radius, sigma)
    assert got.dtype == np.int32 and [int(v) for v in got] == want
    raw = (C.c_int32 * 17)(*([-1] * 17))
    assert _lib.load().fpng_amd_blur_weights(radius, sigma, C.byref(raw)) == 0
    assert list(raw) == want + [0] * (16 - radius)  # (the rest 0)
    assert all(v >= 0 for v in want) and all(a >= b for a, b in zip(want, want[1:]))
    assert abs(2 * sum(want) - want[0] - (1 << 22)) <= radius
    post = {"blur": (radius, sigma)}
    for value in (255, 0):  # a flat plane stays flat
        flat = np.full((radius + 2, radius + 1), value, dtype=np.uint8)
        assert (fpng_amd.view_post_apply(_record(post), flat) == value).all() and (PM.apply_plane(post, flat) == value).all()


# ---- the host twin against the model ----
def _flag_combinations(radius, k):
    """every combination of the three flags, the parameters varied with k"""
    for blur, sol, pos in itertools.product((False, True), repeat=3):
        post = {}
        if blur:
            post["blur"] = (radius, SIGMAS[1 + k % 4] if radius > 1 else (0.5, 2.0)[k & 1])
        if sol:
            post["solarize"] = (128, 0, 255, 1, 77)[k % 5]
        if pos:
            post["posterize"] = (4, 1, 8, 0, 7)[k % 5]
        k += 1
        yield post


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s[0])
def test_the_host_twin_is_the_model(built_lib, shape):
    (w, h), radii = shape
    k = 0
    for radius in radii:
        for name, plane in _planes(w, h, 31 + w).items():
            for post in _flag_combinations(radius, k):
                k += 3
                got = fpng_amd.view_post_apply(_record(post), plane)
                assert got.dtype == np.uint8 and got.shape == plane.shape
                assert np.array_equal(got, PM.apply_plane(post, plane)), (name, post)
    assert np.array_equal(fpng_amd.view_post_apply(fpng_amd.view_post(), plane), plane)  # (no flag: the plane)


# ---- the point operations against Pillow ----
def test_solarize_and_posterize_are_pillows(built_lib):
    from PIL import Image, ImageOps
    every = np.arange(256, dtype=np.uint8).reshape(16, 16)
    noise = np.random.default_rng(5).integers(0, 256, size=(33, 129), dtype=np.uint8)
    for plane in (every, noise):
        img = Image.fromarray(plane, mode="L")
        for threshold in (0, 1, 128, 255):
            want = np.asarray(ImageOps.solarize(img, threshold))
            assert np.array_equal(fpng_amd.view_post_apply(fpng_amd.view_post(solarize=threshold), plane), want), threshold
            assert np.array_equal(PM.apply_plane({"solarize": threshold}, plane), want), threshold
        for bits in range(1, 9):
            want = np.asarray(ImageOps.posterize(img, bits))
            assert np.array_equal(fpng_amd.view_post_apply(fpng_amd.view_post(posterize=bits), plane), want), bits
            assert np.array_equal(PM.apply_plane({"posterize": bits}, plane), want), bits
        assert (fpng_amd.view_post_apply(fpng_amd.view_post(posterize=0), plane) == 0).all()
        # both: solarize first
        want = np.asarray(ImageOps.posterize(ImageOps.solarize(img, 100), 3))
        assert np.array_equal(fpng_amd.view_post_apply(fpng_amd.view_post(solarize=100, posterize=3), plane), want)


# ---- the blur against an independent one ----
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s[0])
def test_the_blur_against_a_double_precision_blur(built_lib, shape):
    """scipy.ndimage.correlate1d(mode="mirror") on both axes with the real-valued weights p / ww, rounded ONCE.  Each pass of the rule
    is within 0.5 + 255 * 33 * 2^-23 of its real value (the byte's rounding, and 33 weights each within 2^-23 of theirs), the
    second pass averages the first one's error with weights that sum to 1, and the comparator rounds once more: a sample differs by
    at most 1.  A shifted or asymmetric kernel or a wrong border would show as a larger difference or a signed mean."""
    import math
    from scipy.ndimage import correlate1d
    (w, h), radii = shape
    for radius in radii:
        for sigma in ((0.5, 2.0) if radius == 1 else (1.3, 2.0, 5.0)):
            p = [math.exp(-0.5 * (d / sigma) ** 2) for d in range(radius + 1)]
            taps = np.array(p[:0:-1] + p, dtype=np.float64)
            taps /= taps.sum()
            for name, plane in _planes(w, h, 77 + radius).items():
                real = correlate1d(correlate1d(plane.astype(np.float64), taps, axis=1, mode="mirror"), taps, axis=0, mode="mirror")
                want = np.clip(np.rint(real), 0, 255).astype(np.int32)
                got = fpng_amd.view_post_apply(fpng_amd.view_post(blur=(2 * radius + 1, sigma)), plane).astype(np.int32)
                diff = got - want
                share, mean = float(np.count_nonzero(diff)) / diff.size, float(diff.mean())
                print(f"{w}x{h} R={radius} sigma={sigma} {name}: max {int(np.abs(diff).max())} share {share:.4f} mean {mean:+.4f}")
                assert np.abs(diff).max() <= 1, (radius, sigma, name)
                assert share <= 0.25, (radius, sigma, name, share)
                assert abs(mean) <= 0.05, (radius, sigma, name, mean)


# ---- refusals ----
def _arrays(records, counts, hwc, chans=3):
    """(files, view_count, crops, views, dests, colors, posts, results): empty destination fields in `files`, identity matrices,
    records without flags"""
    total, n = len(records), len(counts)
    files, cnt = (_lib.PngPlanarIn * n)(), (C.c_uint32 * n)(*counts)
    c, v, d = (_lib.Crop * total)(), (_lib.ResizeView * total)(), ((_lib.ViewDestHwc if hwc else _lib.ViewDest) * total)()
    col, post = (_lib.ViewColor * total)(), (_lib.ViewPost * total)()
    for k, (crop, view) in enumerate(records):
        c[k].x, c[k].y, c[k].w, c[k].h = crop
        v[k].full_w, v[k].full_h, v[k].x, v[k].y, v[k].w, v[k].h, v[k].flags, v[k].filter = view
        for ch in range(3):
            col[k].m[ch][ch] = 1.0
    for f in files:
        f.num_chans = chans
    return files, cnt, c, v, d, col, post, (_lib.DecodeResult * n)()


BLUR, SOLARIZE, POSTERIZE = _lib.POST_BLUR, _lib.POST_SOLARIZE, _lib.POST_POSTERIZE
# (flags, radius, sigma, threshold, bits, reserved) and a piece of the message; the record's view is GOOD[1]: a 6 x 4 window
BAD_RECORDS = [((8, 0, 0.0, 0, 0, (0, 0)), "flags"), ((0x80000000 | BLUR, 1, 1.0, 0, 0, (0, 0)), "flags"),
               ((0, 0, 0.0, 0, 0, (1, 0)), "reserved"), ((SOLARIZE, 0, 0.0, 3, 0, (0, 7)), "reserved"),
               ((BLUR, 0, 1.0, 0, 0, (0, 0)), "blur_radius must be 1 .. 16"), ((BLUR, 17, 1.0, 0, 0, (0, 0)), "blur_radius must be 1 .. 16"),
               ((BLUR, 0xFFFFFFFF, 1.0, 0, 0, (0, 0)), "blur_radius must be 1 .. 16"),
               ((BLUR, 1, 0.0, 0, 0, (0, 0)), "blur_sigma"), ((BLUR, 1, -1.0, 0, 0, (0, 0)), "blur_sigma"), ((BLUR, 1, float("nan"), 0, 0, (0, 0)), "blur_sigma"),
               ((BLUR, 1, float("inf"), 0, 0, (0, 0)), "blur_sigma"), ((BLUR, 1, -0.0, 0, 0, (0, 0)), "blur_sigma"),
               ((BLUR, 4, 1.0, 0, 0, (0, 0)), "below the window"), ((BLUR, 16, 1.0, 0, 0, (0, 0)), "below the window"),
               ((0, 1, 0.0, 0, 0, (0, 0)), "without FPNG_AMD_POST_BLUR"), ((SOLARIZE, 0, 1.0, 0, 0, (0, 0)), "without FPNG_AMD_POST_BLUR"),
               ((POSTERIZE, 0, float("nan"), 0, 0, (0, 0)), "without FPNG_AMD_POST_BLUR"),
               ((SOLARIZE, 0, 0.0, 256, 0, (0, 0)), "solarize_threshold must be 0 .. 255"), ((POSTERIZE, 0, 0.0, 0, 9, (0, 0)), "posterize_bits must be 0 .. 8"),
               ((POSTERIZE, 0, 0.0, 5, 3, (0, 0)), "without FPNG_AMD_POST_SOLARIZE"), ((0, 0, 0.0, 255, 0, (0, 0)), "without FPNG_AMD_POST_SOLARIZE"),
               ((SOLARIZE, 0, 0.0, 5, 3, (0, 0)), "without FPNG_AMD_POST_POSTERIZE"), ((BLUR, 1, 1.0, 0, 8, (0, 0)), "without FPNG_AMD_POST_POSTERIZE")]
GOOD_RECORDS = [(0, 0, 0.0, 0, 0, (0, 0)), (BLUR, 3, 0.1, 0, 0, (0, 0)), (BLUR, 1, 1.0e300, 0, 0, (0, 0)), (SOLARIZE, 0, 0.0, 0, 0, (0, 0)), (SOLARIZE, 0, 0.0, 255, 0, (0, 0)),
                (POSTERIZE, 0, 0.0, 0, 0, (0, 0)), (POSTERIZE, 0, 0.0, 0, 8, (0, 0)), (BLUR | SOLARIZE | POSTERIZE, 2, 5.0, 128, 4, (0, 0))]


def _fill(rec, values):
    rec.flags, rec.blur_radius, rec.blur_sigma, rec.solarize_threshold, rec.posterize_bits = values[:5]
    rec.reserved[0], rec.reserved[1] = values[5]


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
        return _arrays([GOOD[0], GOOD[1], GOOD[2]], [2, 1], hwc)

    files, cnt, c, v, d, col, post, res = fresh()
    assert fn(None, files, 2, cnt, c, v, d, col, post, None, res) == -1 and "null/empty batch" in why(), why()  # (nothing is at fault -- the batch has no encoder)
    assert fn(None, files, 2, cnt, c, v, d, col, post, C.byref(fmt), res) == -1 and "null/empty batch" in why(), why()
    assert fn(None, files, 2, cnt, c, v, d, None, post, None, res) == -1 and "null/empty batch" in why(), why()  # (NULL colors: the identity)
    assert fn(None, files, 2, cnt, c, v, d, col, None, None, res) == -1 and "null posts" in why(), why()
    assert fn(None, files, 2, cnt, c, v, d, None, None, None, res) == -1 and "null posts" in why(), why()
    # ---- the records ----
    for colors in (True, False):
        for values, piece in BAD_RECORDS:
            files, cnt, c, v, d, col, post, res = fresh()
            _fill(post[1], values)
            assert fn(None, files, 2, cnt, c, v, d, col if colors else None, post, None, res) == -1 and "fpng_amd_view_post" in why() and piece in why(), (values, why())
        for values in GOOD_RECORDS:
            files, cnt, c, v, d, col, post, res = fresh()
            _fill(post[1], values)
            assert fn(None, files, 2, cnt, c, v, d, col if colors else None, post, None, res) == -1 and "null/empty batch" in why(), (values, why())
    # (R against the window: 3 x 2 takes R = 1, 1 x 1 takes none; the last record of the call is judged too)
    for at, radius, ok in ((0, 1, True), (0, 2, False), (2, 1, False)):
        files, cnt, c, v, d, col, post, res = fresh()
        _fill(post[at], (BLUR, radius, 1.0, 0, 0, (0, 0)))
        assert fn(None, files, 2, cnt, c, v, d, col, post, None, res) == -1 and ("null/empty batch" if ok else "below the window") in why(), (at, radius, why())
    # ---- everything the colour call refuses ----
    files, cnt, c, v, d, col, post, res = fresh()
    _fill(post[0], GOOD_RECORDS[-1][:1] + (1,) + GOOD_RECORDS[-1][2:])
    col[2].m[1][1] = float("nan")
    assert fn(None, files, 2, cnt, c, v, d, col, post, None, res) == -1 and "fpng_amd_view_color::m" in why(), why()
    col[2].m[1][1], col[2].flags = 1.0, 1
    assert fn(None, files, 2, cnt, c, v, d, col, post, None, res) == -1 and "fpng_amd_view_color::flags" in why(), why()
    col[2].flags = 0
    good = [files, 2, cnt, c, v, d, col, post, None, res]
    assert fn(None, *good) == -1 and "null/empty batch" in why(), why()
    for k in (0, 2, 3, 4, 5, 9):  # a null array
        args = list(good)
        args[k] = None
        assert fn(None, *args) == -1 and "null files, view_count, crops, views, dests or results" in why(), (k, why())
    for counts in ([0, 3], [3, 0]):
        assert fn(None, files, 2, (C.c_uint32 * 2)(*counts), c, v, d, col, post, None, res) == -1 and "view_count of 0" in why(), (counts, why())
    v[1].filter = 2
    assert fn(None, *good) == -1 and "filter" in why(), why()
    v[1].filter = 1
    files[1].row_pitch = 4
    assert fn(None, *good) == -1 and "must be NULL / 0" in why(), why()
    files[1].row_pitch = 0
    fmt.dtype = 3
    assert fn(None, files, 2, cnt, c, v, d, col, post, C.byref(fmt), res) == -1 and "null/empty batch" in why(), why()  # (fmt: judged with the encoder's batch)


def test_the_host_functions_refuse_what_the_calls_refuse(built_lib):
    lib = _lib.load()
    k = (C.c_int32 * 17)()
    for radius, sigma in ((0, 1.0), (17, 1.0), (1, 0.0), (1, float("nan")), (1, float("inf")), (2, -3.0)):
        assert lib.fpng_amd_blur_weights(radius, sigma, C.byref(k)) == -1, (radius, sigma)
    plane = np.zeros((4, 6), dtype=np.uint8)
    with pytest.raises(fpng_amd.FpngAmdError, match="below the window"):
        fpng_amd.view_post_apply(fpng_amd.view_post(blur=(9, 1.0)), plane)
    rec = fpng_amd.view_post(solarize=3)
    rec.solarize_threshold = 256
    with pytest.raises(fpng_amd.FpngAmdError, match="solarize_threshold"):
        fpng_amd.view_post_apply(rec, plane)


# ---- the Python door ----
def test_view_post():
    r = fpng_amd.view_post()
    assert (r.flags, r.blur_radius, r.blur_sigma, r.solarize_threshold, r.posterize_bits, list(r.reserved)) == (0, 0, 0.0, 0, 0, [0, 0])
    r = fpng_amd.view_post(blur=(23, 1.5), solarize=128, posterize=4)
    assert (r.flags, r.blur_radius, r.blur_sigma, r.solarize_threshold, r.posterize_bits) == (7, 11, 1.5, 128, 4)
    r = fpng_amd.view_post(solarize=0, posterize=0)  # (0 is a value, not "none")
    assert (r.flags, r.solarize_threshold, r.posterize_bits) == (6, 0, 0)
    assert fpng_amd.view_post(blur=(3, 0.1)).blur_radius == 1 and fpng_amd.view_post(blur=(33, 0.1)).blur_radius == 16
    for bad in ({"blur": (4, 1.0)}, {"blur": (1, 1.0)}, {"blur": (35, 1.0)}, {"blur": 3}, {"blur": (3.5, 1.0)}, {"solarize": 256}, {"solarize": -1}, {"solarize": 1.5},
                {"posterize": 9}, {"posterize": -1}):
        with pytest.raises(ValueError):
            fpng_amd.view_post(**bad)


@pytest.mark.parametrize("hwc", [False, True])
def test_the_post_keyword_shapes_and_lengths(hwc):
    """make_decode_batch_views(_hwc)(..., post=) needs no GPU: one record, one per file, one per view; wrong lengths and types raise"""
    make = Encoder.make_decode_batch_views_hwc if hwc else Encoder.make_decode_batch_views
    pngs = [b"x" * 8, b"y" * 8]
    crops = [[(0, 0, 8, 8), (1, 1, 4, 4)], [(0, 0, 8, 8)]]
    outs = [[torch.empty((4, 4, 3) if hwc else (3, 4, 4), dtype=torch.uint8) for _ in cs] for cs in crops]
    a, b = fpng_amd.view_post(blur=(3, 1.0)), fpng_amd.view_post(solarize=9)
    assert make(pngs, crops, outs, (4, 4)).posts is None
    db = make(pngs, crops, outs, (4, 4), post=a)
    assert db.colors is None and [(p.flags, p.blur_radius) for p in db.posts] == [(1, 1)] * 3
    db = make(pngs, crops, outs, (4, 4), post=[a, b])
    assert [p.flags for p in db.posts] == [1, 1, 2]
    db = make(pngs, crops, outs, (4, 4), post=[[b, a], [fpng_amd.view_post()]], color=np.eye(3, 4))
    assert db.colors is not None and [p.flags for p in db.posts] == [2, 1, 0]
    for bad in ([a], [a, b, a], [[a], [b]], [[a, b, a], b], [[a, b], []], 3, [a, 3], [[a, {"blur": 1}], b], "ab"):
        with pytest.raises(ValueError):
            make(pngs, crops, outs, (4, 4), post=bad)
