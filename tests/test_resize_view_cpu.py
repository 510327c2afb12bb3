"""No-GPU tests of the resize VIEW interface (fpng_amd_decode_batch(_device)_planar_resize_view, fpng_amd_resize_weights_filter,
fpng_amd_resize_view_source): the exported symbols and the fpng_amd_resize_view record, the refusals that need no device, the
library's bicubic weights against the Python restatement of the rule (resize_view_model.py), that restatement against Pillow itself
(Image.BICUBIC, and a centre window as a slice of Pillow's whole result), the source box against the restatement, center_crop_view's
arithmetic, and the descriptor make_decode_batch_resize_view builds from CPU tensor views."""
import ctypes as C

import numpy as np
import pytest
import torch

import fpng_amd
from fpng_amd import _lib
from fpng_amd.api import Encoder

import resize_model as RM
import resize_view_model as VM
from test_resize_cpu import DTYPES, GRID, NAMED, _pairs

NAMES = ("fpng_amd_decode_batch_planar_resize_view", "fpng_amd_decode_batch_device_planar_resize_view", "fpng_amd_resize_weights_filter",
         "fpng_amd_resize_view_source")


def test_entry_points_and_record(built_lib):
    lib = _lib.load()
    for name in NAMES:
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None
    assert lib.fpng_amd_abi_version() == 5  # (new entry points, the same ABI version)
    assert C.sizeof(_lib.ResizeView) == 32
    assert {n: getattr(_lib.ResizeView, n).offset for n, _ in _lib.ResizeView._fields_} == {
        "full_w": 0, "full_h": 4, "x": 8, "y": 12, "w": 16, "h": 20, "flags": 24, "filter": 28}
    assert (_lib.FILTER_BILINEAR, _lib.FILTER_BICUBIC) == (fpng_amd.FILTER_BILINEAR, fpng_amd.FILTER_BICUBIC) == (0, 1)
    assert C.sizeof(_lib.Resize) == 16  # (the plain resize call's record is what it was)


def _records(crop, view):
    c, v = (_lib.Crop * 1)(), (_lib.ResizeView * 1)()
    c[0].x, c[0].y, c[0].w, c[0].h = crop
    v[0].full_w, v[0].full_h, v[0].x, v[0].y, v[0].w, v[0].h, v[0].flags, v[0].filter = view
    return c, v


# (crop, view (full_w, full_h, x, y, w, h, flags, filter), a word of the refusal's message)
BAD = [((0, 0, 0, 64), (6, 4, 0, 0, 6, 4, 0, 0), "empty crop"), ((0, 0, 96, 0), (6, 4, 0, 0, 6, 4, 0, 1), "empty crop"),
       ((0, 0, 96, 64), (0, 4, 0, 0, 6, 4, 0, 0), "full_w"), ((0, 0, 96, 64), (6, 0, 0, 0, 6, 4, 0, 0), "full_h"),
       ((0, 0, 96, 64), (6, 4, 0, 0, 0, 4, 0, 0), "empty window"), ((0, 0, 96, 64), (6, 4, 0, 0, 6, 0, 0, 1), "empty window"),
       ((0, 0, 96, 64), (6, 4, 1, 0, 6, 4, 0, 0), "x + w"), ((0, 0, 96, 64), (6, 4, 0, 3, 6, 2, 0, 0), "y + h"),
       ((0, 0, 96, 64), (6, 4, 0xFFFFFFFF, 0, 2, 4, 0, 0), "x + w"), ((0, 0, 96, 64), (6, 4, 0, 0xFFFFFFFE, 6, 3, 0, 1), "y + h"),  # (64 bits: no wrap)
       ((0, 0, 96, 64), (6, 4, 0, 0, 6, 4, 2, 0), "flags"), ((0, 0, 96, 64), (6, 4, 0, 0, 6, 4, 0x80000001, 1), "flags"),
       ((0, 0, 96, 64), (6, 4, 0, 0, 6, 4, 0, 2), "filter"), ((0, 0, 96, 64), (6, 4, 0, 0, 6, 4, 1, 0xFFFFFFFF), "filter"),
       ((0, 0, 97, 64), (3, 2, 0, 0, 3, 2, 0, 0), "32"), ((0, 0, 96, 65), (3, 2, 0, 0, 1, 1, 1, 0), "32"),
       ((0, 0, 97, 64), (6, 4, 0, 0, 6, 4, 0, 1), "16"), ((0, 0, 96, 65), (6, 4, 5, 3, 1, 1, 0, 1), "16"),
       ((0, 0, 96, 64), (3, 2, 0, 0, 3, 2, 0, 1), "16")]  # (32 x: bilinear's limit, past bicubic's)
GOOD = [((0, 0, 96, 64), (3, 2, 0, 0, 3, 2, 0, 0)), ((0, 0, 96, 64), (6, 4, 0, 0, 6, 4, 1, 1)), ((0, 0, 96, 64), (6, 4, 5, 3, 1, 1, 0, 1)),
        ((7, 9, 1, 1), (0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFE, 0, 1, 0xFFFFFFFF, 0, 0))]


def test_invalid_arguments_are_refused_without_a_device(built_lib):
    """The records are judged before anything else, so with no encoder at all every call returns -1 -- and the message names the
    reason: a bad record its own, a good one only the missing encoder"""
    lib = _lib.load()
    fmt = _lib.FloatFormat()

    def why():
        return lib.fpng_amd_last_error().decode()

    good_c, good_v = _records(*GOOD[0])
    for fn in (lib.fpng_amd_decode_batch_planar_resize_view, lib.fpng_amd_decode_batch_device_planar_resize_view):
        assert fn(None, None, None, good_v, 1, None, None) == -1 and "null crops" in why()
        assert fn(None, None, good_c, None, 1, C.byref(fmt), None) == -1 and "null views" in why()
        for crop, view, word in BAD:
            c, v = _records(crop, view)
            assert fn(None, None, c, v, 1, None, None) == -1 and word in why(), (crop, view, why())
        for crop, view in GOOD:  # (no record is at fault -- the batch has no encoder)
            c, v = _records(crop, view)
            assert fn(None, None, c, v, 1, None, None) == -1 and "null/empty batch" in why(), (crop, view, why())
    # the source box: the same judgement of a record
    box = _lib.Crop()
    for crop, view, word in BAD:
        c, v = _records(crop, view)
        assert lib.fpng_amd_resize_view_source(c, v, C.byref(box)) == -1 and word in why(), (crop, view, why())
    c, v = _records(*GOOD[1])
    assert lib.fpng_amd_resize_view_source(None, v, C.byref(box)) == -1 and "null" in why()
    assert lib.fpng_amd_resize_view_source(c, None, C.byref(box)) == -1 and "null" in why()
    assert lib.fpng_amd_resize_view_source(c, v, None) == -1 and "null" in why()
    assert lib.fpng_amd_resize_view_source(c, v, C.byref(box)) == 0 and (box.x, box.y, box.w, box.h) == (0, 0, 96, 64)
    # the weights
    u, i = C.c_uint32(), C.c_int32()
    assert lib.fpng_amd_resize_weights_filter(4, 2, 1, None, C.byref(u), C.byref(i)) == -1
    assert lib.fpng_amd_resize_weights_filter(4, 2, 1, C.byref(u), None, C.byref(i)) == -1
    assert lib.fpng_amd_resize_weights_filter(4, 2, 1, C.byref(u), C.byref(u), None) == -1
    w65 = (C.c_int32 * (2 * 65))()
    u2 = (C.c_uint32 * 2)()
    assert lib.fpng_amd_resize_weights_filter(4, 2, 2, u2, u2, w65) == -1 and "filter" in why()
    for bad in ((0, 1, "bicubic"), (1, 0, "bicubic"), (17, 1, "bicubic"), (33, 2, "bicubic"), (33, 1, "bilinear"), (4, 2, 2)):
        with pytest.raises(fpng_amd.FpngAmdError) as e:
            fpng_amd.resize_weights(*bad)
        assert e.value.code == -1, bad
    with pytest.raises(ValueError):
        fpng_amd.resize_weights(4, 2, "lanczos")


def test_the_plain_resize_call_still_refuses_other_flag_bits(built_lib):
    lib = _lib.load()
    c, s = (_lib.Crop * 1)(), (_lib.Resize * 1)()
    c[0].x, c[0].y, c[0].w, c[0].h = 0, 0, 96, 64
    s[0].out_w, s[0].out_h, s[0].flags, s[0].reserved = 3, 2, 2, 0
    for fn in (lib.fpng_amd_decode_batch_planar_resize, lib.fpng_amd_decode_batch_device_planar_resize):
        assert fn(None, None, c, s, 1, None, None) == -1 and "flags" in lib.fpng_amd_last_error().decode()


def test_bilinear_weights_are_the_plain_calls(built_lib):
    for in_size, out_size in _pairs():
        a, b = fpng_amd.resize_weights(in_size, out_size), fpng_amd.resize_weights(in_size, out_size, "bilinear")
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), (in_size, out_size)
        first, count, weights = fpng_amd.resize_weights(in_size, out_size, fpng_amd.FILTER_BILINEAR)
        assert np.array_equal(first, a[0]) and np.array_equal(count, a[1]) and np.array_equal(weights, a[2])
        # (through the entry point that takes a filter, too)
        f2, c2, w2 = np.zeros_like(a[0]), np.zeros_like(a[1]), np.zeros_like(a[2])
        assert _lib.load().fpng_amd_resize_weights_filter(in_size, out_size, 0, f2.ctypes.data_as(C.POINTER(C.c_uint32)), c2.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                          w2.ctypes.data_as(C.POINTER(C.c_int32))) == 0
        assert np.array_equal(f2, a[0]) and np.array_equal(c2, a[1]) and np.array_equal(w2, a[2]), (in_size, out_size)
        mf, mc, mk = VM.axis_weights(in_size, out_size, "bilinear")
        assert (mf, mc, mk) == RM.axis_weights(in_size, out_size)  # (the restatement with a filter is the restatement without)


def test_bicubic_weights_against_the_rule(built_lib):
    """first, count and every weight of fpng_amd_resize_weights_filter(BICUBIC) equal the restatement's; behind a row's count the
    weights are 0; a row sums to 2^22 within `count` units and has at most 65 taps; negative weights exist; 16 x is the limit"""
    pairs = [(a, b) for a, b in _pairs() if a <= 16 * b]
    assert len(pairs) >= 250
    pairs += [(112, 7), (3584, 224), (1600, 100), (500, 341), (375, 256)]  # (exactly 16 x: in = 16 * out is accepted)
    for a, b in ((a, b) for a in GRID for b in GRID if a > 16 * b):  # (past the limit: refused, not computed)
        with pytest.raises(fpng_amd.FpngAmdError):
            fpng_amd.resize_weights(a, b, "bicubic")
    for out_size in (1, 7, 100):
        with pytest.raises(fpng_amd.FpngAmdError):
            fpng_amd.resize_weights(16 * out_size + 1, out_size, "bicubic")
    negative, most, most_abs, limit_abs = 0, 0, 0.0, 0.0
    for in_size, out_size in pairs:
        first, count, weights = fpng_amd.resize_weights(in_size, out_size, "bicubic")
        mf, mc, mk = VM.axis_weights(in_size, out_size, "bicubic")
        assert first.tolist() == mf and count.tolist() == mc, (in_size, out_size)
        assert weights.shape == (out_size, VM.MAX_TAPS)
        for o in range(out_size):
            n = mc[o]
            assert 1 <= n <= VM.MAX_TAPS and mf[o] + n <= in_size, (in_size, out_size, o)
            assert weights[o, :n].tolist() == mk[o], (in_size, out_size, o)
            assert not weights[o, n:].any()
            assert abs(sum(mk[o]) - (1 << 22)) <= n, (in_size, out_size, o, sum(mk[o]))
            negative += min(mk[o]) < 0
            most = max(most, n)
            most_abs = max(most_abs, sum(abs(v) for v in mk[o]) / (1 << 22))
            if in_size == 16 * out_size:
                limit_abs = max(limit_abs, sum(abs(v) for v in mk[o]) / (1 << 22))
    assert negative > 0 and most == 64  # (64 taps at exactly 16 x)
    # a pass's sum stays inside int32: the magnitudes sum to 1.167 * 2^22 at the scale limit (the cubic's lobes: 1 + 4 / 24) and to
    # at most 1.27 * 2^22 anywhere (few taps near in == out, 1.25 at half a sample's phase, a little more where an edge cuts taps)
    assert limit_abs <= 1.17 and most_abs <= 1.3 and 255 * most_abs * (1 << 22) + (1 << 21) < 1 << 31
    # in == out: the identity
    first, count, weights = fpng_amd.resize_weights(49, 49, "bicubic")
    assert all(weights[o, int(np.argmax(weights[o]))] == 1 << 22 and weights[o].sum() == 1 << 22 and not (weights[o] < 0).any() for o in range(49))
    assert [int(first[o] + np.argmax(weights[o])) for o in range(49)] == list(range(49))


def test_the_restatement_is_pillows_bicubic():
    """resize_view_model.resize_plane(.., "bicubic") == Image.fromarray(p, "L").resize((ow, oh), Image.BICUBIC), byte for byte: seeded
    noise and two-level (0 / 255) planes at the named sizes and 100 seeded ones (the draws of test_the_restatement_is_pillows_resize);
    on the two-level planes the unclamped sums leave 0 .. 255 at both ends, so the clamp is exercised"""
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(7)
    cases = list(NAMED) + [((int(rng.integers(1, 90)), int(rng.integers(1, 90))), (int(rng.integers(1, 70)), int(rng.integers(1, 70)))) for _ in range(100)]
    below = above = 0
    for (w, h), (ow, oh) in cases:
        if w > 16 * ow or h > 16 * oh:  # (past the bicubic limit: 4000 x 3 -> 3 x 2 and the like)
            continue
        for kind in ("noise", "levels"):
            p = rng.integers(0, 256, (h, w), dtype=np.uint8)
            if kind == "levels":
                p = ((p & 1) * 255).astype(np.uint8)
            want = np.asarray(Image.fromarray(p, "L").resize((ow, oh), Image.BICUBIC))
            got = VM.resize_plane(p, ow, oh, "bicubic")
            assert got.shape == (oh, ow) and np.array_equal(got, want), ((w, h), (ow, oh), kind, int((got != want).sum()))
            if kind == "levels":
                for sums in (VM.one_pass_sums(p, ow, "bicubic"), VM.one_pass_sums(np.ascontiguousarray(VM.one_pass(p, ow, "bicubic").T), oh, "bicubic")):
                    below += int(((sums >> VM.PRECISION_BITS) < 0).sum())
                    above += int(((sums >> VM.PRECISION_BITS) > 255).sum())
    assert below > 0 and above > 0
    px = rng.integers(0, 256, (3, 33, 47), dtype=np.uint8)
    r = VM.view_planes(px, (20, 9), (3, 2, 11, 5), "bicubic", mirror=True)
    assert np.array_equal(r[1, :, ::-1], VM.resize_plane(px[1], 20, 9, "bicubic")[2:7, 3:14])


def test_a_centre_window_is_a_slice_of_pillows_whole_image():
    """an RGB 500 x 375 image -> 341 x 256 in both filters: the restatement is Pillow's image, and the window (58, 16, 224, 224) of
    view_planes its slice"""
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(11)
    img = rng.integers(0, 256, (375, 500, 3), dtype=np.uint8)
    img[100:200, 150:300] = (img[100:200, 150:300] & 1) * 255  # (a two-level patch inside the window's pre-image)
    px = np.ascontiguousarray(img.transpose(2, 0, 1))
    crop, full, window = fpng_amd.center_crop_view(500, 375, 256, 224)
    assert (crop, full, window) == ((0, 0, 500, 375), (341, 256), (58, 16, 224, 224))
    for name, pil in (("bilinear", Image.BILINEAR), ("bicubic", Image.BICUBIC)):
        want = np.asarray(Image.fromarray(img, "RGB").resize(full, pil)).transpose(2, 0, 1)
        assert np.array_equal(VM.view_planes(px, full, None, name), want), name
        assert np.array_equal(VM.view_planes(px, full, window, name), want[:, 16:240, 58:282]), name
    assert VM.view_source(crop, full, window, "bicubic")[::2] == (83, 333)  # (columns 83 up to, not including, 416 of 500)
    assert VM.view_source(crop, full, window, "bilinear")[::2] == (84, 330)  # (84 up to 414)


def _tight(in_size, out_size, o0, n, begin, end, filter):
    """begin .. end holds every tap of samples o0 .. o0 + n - 1, and its first and last sample are taps (a position inside some
    sample's first .. first + count) -- dropping either would lose one"""
    first, count, _ = VM.axis_weights(in_size, out_size, filter)
    spans = [(first[o], first[o] + count[o]) for o in range(o0, o0 + n)]
    return all(begin <= a and b <= end for a, b in spans) and any(a <= begin < b for a, b in spans) and any(a <= end - 1 < b for a, b in spans)


def test_view_source_against_the_model(built_lib):
    cases = [(crop, full, window, f) for views in VM.VIEWS.values() for crop, full, window, fs in views for f in fs]
    rng = np.random.default_rng(5)
    while len(cases) < 200 + sum(len(fs) for views in VM.VIEWS.values() for *_, fs in views):
        f = VM.FILTERS[int(rng.integers(0, 2))]
        cw, ch = int(rng.integers(1, 700)), int(rng.integers(1, 500))
        fw, fh = int(rng.integers(1, 400)), int(rng.integers(1, 300))
        if cw > VM.MAX_SCALE[f] * fw or ch > VM.MAX_SCALE[f] * fh:
            continue
        w, h = int(rng.integers(1, fw + 1)), int(rng.integers(1, fh + 1))
        cases.append(((int(rng.integers(0, 5000)), int(rng.integers(0, 5000)), cw, ch), (fw, fh), (int(rng.integers(0, fw - w + 1)), int(rng.integers(0, fh - h + 1)), w, h), f))
    smaller = 0
    for crop, full, window, f in cases:
        box = fpng_amd.resize_view_source(crop, full, window, f)
        assert box == VM.view_source(crop, full, window, f), (crop, full, window, f)
        x, y, w, h = (0, 0) + full if window is None else window
        assert crop[0] <= box[0] and box[0] + box[2] <= crop[0] + crop[2] and crop[1] <= box[1] and box[1] + box[3] <= crop[1] + crop[3]
        assert _tight(crop[2], full[0], x, w, box[0] - crop[0], box[0] - crop[0] + box[2], f), (crop, full, window, f)
        assert _tight(crop[3], full[1], y, h, box[1] - crop[1], box[1] - crop[1] + box[3], f), (crop, full, window, f)
        smaller += box[2] * box[3] < crop[2] * crop[3]
        if window is None:  # (the whole image needs the whole crop)
            assert box == tuple(crop)
    assert smaller >= 100
    # the evaluation transform of a 500 x 375 file
    crop, full, window = fpng_amd.center_crop_view(500, 375, 256, 224)
    box = fpng_amd.resize_view_source(crop, full, window, "bicubic")
    assert (box[0], box[0] + box[2]) == (83, 416)
    box = fpng_amd.resize_view_source(crop, full, window)  # (bilinear)
    assert (box[0], box[0] + box[2]) == (84, 414)
    with pytest.raises(ValueError):
        fpng_amd.resize_view_source((-1, 0, 5, 5), (5, 5))


def test_a_box_past_the_first_tiles_names_fewer_of_them(built_lib):
    """the view (140, 30, 20, 10) of 600 x 130 -> 300 x 65: its box starts past the first 256-column block and the first 48-row
    segment of the pixel pass, so the crop stage runs fewer tiles than for the crop (test_gpu_resize_view.py checks its bytes)"""
    crop, full, window, fs = VM.VIEWS[(600, 130)][3]
    assert window == (140, 30, 20, 10)
    whole = fpng_amd.crop_tiles(600, 130, crop)
    for f in fs:
        box = fpng_amd.resize_view_source(crop, full, window, f)
        assert box == VM.view_source(crop, full, window, f) and box[0] > 256 and box[1] > 48
        nseg, first, ncb = fpng_amd.crop_tiles(600, 130, box)
        assert first == 1 and ncb == 1 and nseg * ncb < whole[0] * whole[2], (box, (nseg, first, ncb), whole)


def _torchvision(file_w, file_h, resize, crop):
    """Resize(resize) + CenterCrop(crop)'s arithmetic, restated: the shorter side to `resize`, the longer to int(resize * long /
    short); the window's corner by Python's round()"""
    ch, cw = (crop, crop) if isinstance(crop, int) else crop
    short, long = (file_w, file_h) if file_w <= file_h else (file_h, file_w)
    new_short, new_long = resize, int(resize * long / short)
    full_w, full_h = (new_short, new_long) if file_w <= file_h else (new_long, new_short)
    return (0, 0, file_w, file_h), (full_w, full_h), (int(round((full_w - cw) / 2.0)), int(round((full_h - ch) / 2.0)), cw, ch)


def test_center_crop_view():
    assert fpng_amd.center_crop_view(500, 375, 256, 224) == ((0, 0, 500, 375), (341, 256), (58, 16, 224, 224))
    assert fpng_amd.center_crop_view(375, 500, 256, 224) == ((0, 0, 375, 500), (256, 341), (16, 58, 224, 224))
    assert fpng_amd.center_crop_view(1920, 1080, 256, 224) == ((0, 0, 1920, 1080), (455, 256), (116, 16, 224, 224))  # (115.5 rounds to even)
    assert fpng_amd.center_crop_view(300, 300, 256, (224, 200)) == ((0, 0, 300, 300), (256, 256), (28, 16, 200, 224))
    assert fpng_amd.center_crop_view(600, 130, 64, 64) == ((0, 0, 600, 130), (295, 64), (116, 0, 64, 64))  # (115.5 again)
    for args in ((500, 375, 256, 224), (375, 500, 232, (224, 200)), (1280, 720, 342, 299), (97, 64, 65, 64), (64, 64, 64, 64), (1, 7, 3, (5, 3))):
        assert fpng_amd.center_crop_view(*args) == _torchvision(*args), args
    for args in ((500, 375, 200, 224), (500, 375, 256, (224, 400)), (0, 375, 256, 224), (500, 375, 256, 0)):  # (no padding)
        with pytest.raises(ValueError):
            fpng_amd.center_crop_view(*args)


@pytest.mark.parametrize("dtype,e", DTYPES)
def test_descriptor_from_views(built_lib, dtype, e):
    """byte pitches and pixels_cap of window-sized views of a larger canvas; crops, full sizes, windows, filters and mirror flags per
    file or one for all; a destination that is not its window's size is refused"""
    canvas = torch.zeros(4, 3, 300, 400, dtype=dtype)
    crops = [(5, 7, 9, 11), (250, 40, 13, 20), (0, 0, 600, 130), (61, 0, 7, 1)]
    fulls = [(65, 17), (13, 20), (256, 256), (9, 1)]
    windows = [None, (1, 2, 12, 18), (16, 16, 224, 224), (8, 0, 1, 1)]
    sizes = [(65, 17), (12, 18), (224, 224), (1, 1)]  # (w, h) of the destinations
    filters = ["bicubic", "bilinear", fpng_amd.FILTER_BICUBIC, 0]
    outs = [canvas[i, :, 10:10 + oh, 20:20 + ow] for i, (ow, oh) in enumerate(sizes)]
    pngs = [b"\x89PNG" + bytes(60)] * 4  # (host files: only their address and size are recorded)
    mirrors = [False, True, True, False]
    db = Encoder.make_decode_batch_resize_view(pngs, crops, outs, fulls, windows, filters, mirror=mirrors, bottom_up=[False, True, False, False])
    assert isinstance(db, fpng_amd.DecodeBatchResizeView) and not isinstance(db, fpng_amd.DecodeBatchResize) and not db.device_data
    assert (db.fmt is None) == (dtype == torch.uint8)
    if db.fmt is not None:
        assert db.fmt.dtype == fpng_amd.FLOAT_DTYPES[dtype] and db.fmt.reserved == 0
    for i, ((x, y, w, h), (ow, oh)) in enumerate(zip(crops, sizes)):
        r, c, v = db.arr[i], db.crops[i], db.views[i]
        assert (c.x, c.y, c.w, c.h) == (x, y, w, h)
        assert (v.full_w, v.full_h) == fulls[i] and (v.x, v.y, v.w, v.h) == (windows[i] or (0, 0) + fulls[i])
        assert (v.flags, v.filter) == (1 if mirrors[i] else 0, (1, 0, 1, 0)[i])
        rp = 400 * e if oh > 1 else 0
        first = outs[i].data_ptr()
        assert r.num_chans == 3 and r.size == 64
        assert r.plane_pitch == 300 * 400 * e
        assert (r.d_pixels, r.row_pitch) == ((first + (oh - 1) * rp, -rp) if i == 1 else (first, rp))
        assert r.pixels_cap == 2 * 300 * 400 * e + (oh - 1) * abs(rp) + ow * e
    # one full size, window, filter and mirror flag for every file
    batch = torch.zeros(4, 3, 224, 224, dtype=dtype)
    db = Encoder.make_decode_batch_resize_view(pngs, crops, list(batch), (256, 256), (16, 16, 224, 224), "bicubic", mirror=True)
    assert [(v.full_w, v.full_h, v.x, v.y, v.w, v.h, v.flags, v.filter) for v in db.views] == [(256, 256, 16, 16, 224, 224, 1, 1)] * 4
    assert [r.d_pixels for r in db.arr] == [batch[i].data_ptr() for i in range(4)]
    db = Encoder.make_decode_batch_resize_view(pngs, crops, list(batch), (224, 224))  # (no window: the whole; bilinear)
    assert [(v.x, v.y, v.w, v.h, v.flags, v.filter) for v in db.views] == [(0, 0, 224, 224, 0, 0)] * 4
    v = canvas[0, :, :11, :9]
    with pytest.raises(ValueError):  # a destination that is not its window's size
        Encoder.make_decode_batch_resize_view(pngs[:1], crops[:1], [v], (20, 20), (0, 0, 9, 12))
    with pytest.raises(ValueError):  # ... nor, without a window, the full size
        Encoder.make_decode_batch_resize_view(pngs[:1], crops[:1], [v], (9, 12))
    with pytest.raises(ValueError):  # one mirror flag per file
        Encoder.make_decode_batch_resize_view(pngs[:2], crops[:2], [v, v], (9, 11), mirror=[True])
    with pytest.raises(ValueError):  # one full size per file
        Encoder.make_decode_batch_resize_view(pngs[:2], crops[:2], [v, v], [(9, 11)])
    with pytest.raises(ValueError):  # one window per file
        Encoder.make_decode_batch_resize_view(pngs[:2], crops[:2], [v, v], (9, 11), [None, None, None])
    with pytest.raises(ValueError):  # an unknown filter
        Encoder.make_decode_batch_resize_view(pngs[:1], crops[:1], [v], (9, 11), filter="nearest")
    other = torch.zeros(3, 11, 9, dtype=torch.float16 if dtype != torch.float16 else torch.float32)
    with pytest.raises(ValueError):  # mixed dtypes
        Encoder.make_decode_batch_resize_view(pngs[:2], crops[:2], [v, other], (9, 11))
    with pytest.raises(ValueError):  # one crop per file
        Encoder.make_decode_batch_resize_view(pngs[:2], crops[:1], [v, v], (9, 11))
    with pytest.raises(ValueError):
        Encoder.make_decode_batch_resize_view(pngs[:1], [(-1, 0, 9, 11)], [v], (9, 11))
    with pytest.raises(ValueError):
        Encoder.make_decode_batch_resize_view(pngs[:1], crops[:1], [v], (9, 11), (-1, 0, 9, 11))
    if dtype == torch.uint8:
        for kw in ({"mean": (0.5,) * 3, "std": (0.5,) * 3}, {"scale": [1.0]}, {"bias": [0.0]}):
            with pytest.raises(ValueError):  # float arguments with uint8 destinations
                Encoder.make_decode_batch_resize_view(pngs[:1], crops[:1], [v], (9, 11), **kw)
    else:
        db = Encoder.make_decode_batch_resize_view(pngs[:1], [(0, 0, 90, 110)], [v], (9, 11), mean=(0.5,) * 3, std=(0.25,) * 3)
        assert db.fmt.scale[0] == pytest.approx(1 / (255 * 0.25)) and db.fmt.bias[2] == -2.0 and db.fmt.bias[3] == 0.0
