"""CPU tests of the renditions' host side (fpng_amd_encode_submit_renditions, include/fpng_amd.h; no GPU): the host twin
fpng_amd_rendition_pixels -- the text enc_resize_kernel compiles: source accessor, passes, alpha rule -- against Pillow's
crop(box).resize(size, filter) and against rendition_model.py in every source layout, and fpng_amd_renditions_plan, the submit
call's validation, on every refusal, the scale limits and the scratch placement."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image

import fpng_amd
from fpng_amd import _lib

import alpha_model as AM
import rendition_model as RM
from rendition_cases import ex_view, float_tensor, planar_view
from test_float_encode_cpu import IMAGENET_MEAN, IMAGENET_STD, float_image

PIL_FILTER = {"nearest": Image.NEAREST, "box": Image.BOX, "hamming": Image.HAMMING, "lanczos": Image.LANCZOS, "bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC}
INVALID_ARG, BUFFER_TOO_SMALL = -1, -4
# (box, size) of a 67 x 41 image: shrinking both ways, a box growing across a tile border, the identity, a strong reduction, 1 x 1
CASES = [(None, (20, 30)), ((3, 5, 40, 30), (65, 17)), ((1, 1, 9, 9), (9, 9)), ((0, 0, 40, 20), (4, 2)), ((60, 30, 7, 11), (1, 1)), ((66, 40, 1, 1), (5, 3))]


def _noise(w, h, c, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, c), dtype=np.uint8)


def _pillow(img, box, size, filter, alpha):
    """Pillow's answer: crop(box).resize(size, filter) -- of the RGBA image (which premultiplies, except where it does not), or per
    band (the straight rule)"""
    x, y, w, h = box or (0, 0, img.shape[1], img.shape[0])
    im = Image.fromarray(img).crop((x, y, x + w, y + h))
    if img.shape[2] == 4 and alpha is None:
        return np.stack([np.asarray(b.resize(size, PIL_FILTER[filter])) for b in im.split()], axis=-1)
    return np.asarray(im.resize(size, PIL_FILTER[filter]))


def test_entry_points_and_record(built_lib):
    lib = _lib.load()
    for name in ("fpng_amd_encode_submit_renditions", "fpng_amd_renditions_plan", "fpng_amd_rendition_pixels"):
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
    assert lib.fpng_amd_abi_version() == 5  # (new entry points, the same ABI version)
    assert C.sizeof(_lib.Rendition) == 56
    assert {n: getattr(_lib.Rendition, n).offset for n, _ in _lib.Rendition._fields_} == {
        "image": 0, "filter": 4, "box_x": 8, "box_y": 12, "box_w": 16, "box_h": 20, "w": 24, "h": 28, "alpha_op": 32, "reserved": 36, "d_out": 40, "out_cap": 48}
    assert [fpng_amd.RENDITION_FILTERS[f] for f in RM.FILTERS] == [0, 1, 2, 3, 4, 5]


@pytest.mark.parametrize("filter", ["bilinear", "bicubic", "box", "nearest"])
def test_the_twin_is_pillow(built_lib, filter):
    """exact on RGB and on RGBA, straight (Pillow per band) and premultiplied (Pillow's RGBA resize), the identity included -- where
    Pillow returns a copy -- and NEAREST, where it does not premultiply"""
    for img in (_noise(67, 41, 3, 1), AM.pattern(67, 41, seed=2)):
        for box, size in CASES:
            for alpha in (None, "premultiplied") if img.shape[2] == 4 else (None,):
                if not all(RM.scale_ok(i, o, filter) for i, o in zip((box or (0, 0, 67, 41))[2:], size)):
                    continue
                got = fpng_amd.rendition_pixels(img, fpng_amd.rendition(0, size, box, filter, alpha))
                assert np.array_equal(got, _pillow(img, box, size, filter, alpha)), (filter, box, size, alpha)
                assert np.array_equal(got, RM.pixels(img, size, box, filter, alpha)), (filter, box, size, alpha)
    rgba = AM.pattern(67, 41, seed=2)
    if filter != "nearest":  # the two alpha rules differ on this image, and the identity is a copy under either
        r = [fpng_amd.rendition_pixels(rgba, fpng_amd.rendition(0, (20, 30), None, filter, a)) for a in (None, "premultiplied")]
        assert not np.array_equal(r[0], r[1])
    assert np.array_equal(fpng_amd.rendition_pixels(rgba, fpng_amd.rendition(0, (9, 9), (1, 1, 9, 9), filter, "premultiplied")), rgba[1:10, 1:10])


def test_the_twin_is_pillow_on_both_sides_of_the_fused_pass(built_lib):
    """the twin runs the horizontal pass the kernel runs for the record: fused (all channels of a 4-byte source from one load per
    tap) while the tile holds T once per channel within 32 KB of LDS, the channels in turn beyond -- with 64 columns kept and 17
    rows made of 100 .. 120 that bound is crossed between 6 x and 7 x"""
    img = AM.pattern(64, 120, seed=5)
    for in_h in range(100, 121):
        for alpha in (None, "premultiplied"):
            got = fpng_amd.rendition_pixels(img, fpng_amd.rendition(0, (64, 17), (0, 0, 64, in_h), "bilinear", alpha))
            assert np.array_equal(got, _pillow(img, (0, 0, 64, in_h), (64, 17), "bilinear", alpha)), (in_h, alpha)


@pytest.mark.parametrize("filter", ["hamming", "lanczos"])
def test_hamming_and_lanczos_are_the_model_and_pillow_on_these_cases(built_lib, filter):
    """exact against the Python model (whose sin and cos are libm's, the twin's its own text: test_views_resample_cpu.py sweeps the
    weights), and equal to Pillow on these cases, as the decode side states"""
    for img in (_noise(67, 41, 3, 1), AM.pattern(67, 41, seed=2)):
        for box, size in CASES:
            for alpha in (None, "premultiplied") if img.shape[2] == 4 else (None,):
                if not all(RM.scale_ok(i, o, filter) for i, o in zip((box or (0, 0, 67, 41))[2:], size)):
                    continue
                got = fpng_amd.rendition_pixels(img, fpng_amd.rendition(0, size, box, filter, alpha))
                assert np.array_equal(got, RM.pixels(img, size, box, filter, alpha)), (filter, box, size, alpha)
                assert np.array_equal(got, _pillow(img, box, size, filter, alpha)), (filter, box, size, alpha)


SPECS = [((65, 17), None, "bilinear"), ((31, 33), (2, 3, 90, 40), "bicubic"), ((9, 5), (60, 20, 9, 5), "nearest"), ((20, 9), (1, 1, 96, 44), "lanczos"),
         ((40, 20), None, "hamming"), ((50, 50), (96, 44, 1, 1), "box")]


def _twin_is_model(images, img, what, **kw):
    for size, box, f in SPECS:
        for alpha in (None, "premultiplied") if img.shape[2] == 4 else (None,):
            got = fpng_amd.rendition_pixels(images, fpng_amd.rendition(0, size, box, f, alpha), **kw)
            assert np.array_equal(got, RM.pixels(img, size, box, f, alpha)), (what, size, box, f, alpha)


@pytest.mark.parametrize("name", list(fpng_amd.SRC_FORMATS))
def test_the_twin_reads_every_interleaved_format_and_pitch(built_lib, name):
    """every FPNG_AMD_SRC_* format, packed, padded, odd (3-byte sources) and negative pitches; X bytes and padding are noise"""
    _, sb, c = fpng_amd.SRC_FORMATS[name]
    img = _noise(97, 45, c, 20 + c)
    for pk in ["packed", "wide", "neg"] + (["odd"] if sb == 3 else []):
        d, host, view, order, up = ex_view(img, name, pk, np.random.default_rng(8))
        _twin_is_model([view], img, f"{name} {pk}", kind="ex", order=order, bottom_up=up)
        assert np.array_equal(d.numpy(), host)
    if name in ("RGB", "RGBA"):  # the plain kind: R first, tight
        _twin_is_model([torch.from_numpy(img)], img, "image")


@pytest.mark.parametrize("c", [3, 4])
def test_the_twin_reads_planes_with_either_sign_of_either_pitch(built_lib, c):
    img = _noise(97, 45, c, 20 + c)
    for reverse in (False, True):
        d, host, view, order = planar_view(img, reverse, np.random.default_rng(9))
        _twin_is_model([view], img, f"planar, reversed {reverse}", kind="planar", order=order)
        # bottom-up rows: the tensor's row 0 is the image's bottom row
        _twin_is_model([view], np.ascontiguousarray(img[::-1]), f"planar, reversed {reverse}, bottom-up", kind="planar", order=order, bottom_up=True)


@pytest.mark.parametrize("code", [0, 1, 2])
def test_the_twin_quantises_float_planes_first(built_lib, code):
    """f32, f16 and bf16 under the inverse of Normalize(mean, std): the rendition is the resize of the bytes quantize.h's rule gives
    (float_image: the oracle's bytes, no element near a tie)"""
    c = 3 + (code & 1)
    scale, bias = fpng_amd.denormalize_constants(IMAGENET_MEAN, IMAGENET_STD)
    el, img = float_image(_noise(97, 45, c, 30 + code), code, scale, bias, np.random.default_rng(40 + code),
                          to_float=lambda u, ch: (u - IMAGENET_MEAN[ch]) / IMAGENET_STD[ch] if ch < 3 else u)
    _twin_is_model([float_tensor(el, code)], img, f"float {code}", kind="float", mean=IMAGENET_MEAN, std=IMAGENET_STD)
    rev = float_tensor(np.ascontiguousarray(el[..., ::-1]), code)  # planes stored [A,] B, G, R
    _twin_is_model([rev], img, f"float {code}, reversed planes", kind="float", order="abgr" if c == 4 else "bgr", mean=IMAGENET_MEAN, std=IMAGENET_STD)


# ---- fpng_amd_renditions_plan: the submit call's validation ----
def _plan(kind=0, arr=None, n_images=1, fmt=None, r=None, n=1, packed=0, want_offsets=False):
    total, offs = C.c_uint64(0), (C.c_uint64 * max(n, 1))()
    rc = _lib.load().fpng_amd_renditions_plan(kind, C.cast(arr, C.c_void_p) if arr is not None else None, n_images, C.byref(fmt) if fmt is not None else None, r, n, packed,
                                              C.byref(total), offs)
    return (rc, total.value, list(offs)[:n]) if want_offsets else rc


def _images(**kw):
    arr = (_lib.Image * 1)()
    arr[0].d_pixels, arr[0].w, arr[0].h, arr[0].num_chans = 0x10000, 64, 40, 4
    for k, v in kw.items():
        setattr(arr[0], k, v)
    return arr


def _rend(**kw):
    arr = (_lib.Rendition * 1)()
    r = arr[0]
    r.image, r.filter, r.w, r.h, r.d_out, r.out_cap = 0, 0, 20, 10, 0x20000, fpng_amd.max_encoded_size(20, 10, 4)
    for k, v in kw.items():
        setattr(r, k, v)
    return arr


def test_the_plan_returns_every_refusal(built_lib):
    assert _plan(arr=_images(), r=_rend()) == 0
    assert _plan(arr=_images(), r=_rend(d_out=None, out_cap=0), packed=1) == 0
    assert _plan(arr=_images(), r=_rend(box_x=63, box_y=39, box_w=1, box_h=1, w=5, h=5, out_cap=1 << 20)) == 0  # the last pixel
    assert _plan(arr=_images(), r=_rend(alpha_op=2)) == 0
    fmt = _lib.FloatFormat()
    ex = (_lib.ImageEx * 1)()
    ex[0].d_pixels, ex[0].w, ex[0].h, ex[0].format = 0x10000, 64, 40, 0
    pl = (_lib.ImagePlanar * 1)()
    pl[0].d_pixels, pl[0].w, pl[0].h, pl[0].num_chans = 0x10000, 64, 40, 3
    bad = [("unknown kind", INVALID_ARG, dict(kind=4)), ("unknown filter", INVALID_ARG, dict(r=_rend(filter=6))), ("unknown alpha op", INVALID_ARG, dict(r=_rend(alpha_op=3))),
           ("the composite op", INVALID_ARG, dict(r=_rend(alpha_op=1))), ("image >= n_images", INVALID_ARG, dict(r=_rend(image=1))),
           ("box partly zero", INVALID_ARG, dict(r=_rend(box_x=1, box_y=1, box_w=0, box_h=5))), ("box empty", INVALID_ARG, dict(r=_rend(box_w=5))),
           ("box outside, x", INVALID_ARG, dict(r=_rend(box_x=60, box_w=5, box_h=5))), ("box outside, y", INVALID_ARG, dict(r=_rend(box_y=36, box_w=5, box_h=5))),
           ("box outside, wrap", INVALID_ARG, dict(r=_rend(box_x=0xFFFFFFFF, box_w=2, box_h=2))),
           ("w = 0", INVALID_ARG, dict(r=_rend(w=0))), ("h = 0", INVALID_ARG, dict(r=_rend(h=0))), ("h past 2^24", INVALID_ARG, dict(r=_rend(h=(1 << 24) + 1))),
           ("scale, bilinear", INVALID_ARG, dict(r=_rend(w=1))), ("scale, bicubic", INVALID_ARG, dict(r=_rend(filter=1, w=3))), ("scale, lanczos", INVALID_ARG, dict(r=_rend(filter=5, w=5))),
           ("reserved", INVALID_ARG, dict(r=_rend(reserved=1))), ("no renditions", INVALID_ARG, dict(n=0)), ("65536 renditions", INVALID_ARG, dict(n=65536)),
           ("null renditions", INVALID_ARG, dict(r=None)),
           ("d_out with a pack", INVALID_ARG, dict(packed=1)), ("out_cap with a pack", INVALID_ARG, dict(packed=1, r=_rend(d_out=None))),
           ("no d_out without a pack", INVALID_ARG, dict(r=_rend(d_out=None, out_cap=0))), ("d_out misaligned", INVALID_ARG, dict(r=_rend(d_out=0x20008))),
           ("out_cap", BUFFER_TOO_SMALL, dict(r=_rend(out_cap=fpng_amd.max_encoded_size(20, 10, 4) - 1))),
           ("an image's d_out", INVALID_ARG, dict(arr=_images(d_out=0x30000, out_cap=1 << 20))), ("an image's out_cap", INVALID_ARG, dict(arr=_images(out_cap=1))),
           ("fmt with kind image", INVALID_ARG, dict(fmt=fmt)), ("no fmt with kind float", INVALID_ARG, dict(kind=3, arr=pl)), ("no images", INVALID_ARG, dict(n_images=0)),
           ("null images", INVALID_ARG, dict(arr=None)), ("null pixels", INVALID_ARG, dict(arr=_images(d_pixels=None))),
           # the kinds' own rules
           ("RGBA pixels misaligned", INVALID_ARG, dict(arr=_images(d_pixels=0x10002))), ("5 channels", INVALID_ARG, dict(arr=_images(num_chans=5))),
           ("unknown source format", INVALID_ARG, dict(kind=1, arr=(lambda a: (setattr(a[0], "format", 10), a)[1])(_copy(ex)))),
           ("a pitch below the row", INVALID_ARG, dict(kind=1, arr=(lambda a: (setattr(a[0], "row_pitch", 100), a)[1])(_copy(ex)))),
           ("planes that overlap", INVALID_ARG, dict(kind=2, arr=(lambda a: (setattr(a[0], "plane_pitch", 64), a)[1])(_copy(pl)))),
           ("planar reserved", INVALID_ARG, dict(kind=2, arr=(lambda a: (setattr(a[0], "reserved", 1), a)[1])(_copy(pl))))]
    for what, code, kw in bad:
        kw = dict(dict(arr=_images(), r=_rend()), **kw)
        assert _plan(**kw) == code, what
        assert _lib.load().fpng_amd_last_error(), what
    # the same records in the other kinds pass
    assert _plan(kind=1, arr=ex, r=_rend(out_cap=1 << 20)) == 0 and _plan(kind=2, arr=pl, r=_rend(out_cap=1 << 20)) == 0
    fmt.scale[:] = [255.0] * 4
    assert _plan(kind=3, arr=pl, fmt=fmt, r=_rend(out_cap=1 << 20)) == 0
    fmt.dtype = 3
    assert _plan(kind=3, arr=pl, fmt=fmt, r=_rend(out_cap=1 << 20)) == INVALID_ARG


def _copy(arr):
    out = type(arr)()
    C.memmove(out, arr, C.sizeof(arr))
    return out


def test_the_scale_limits_are_pinned_on_both_sides(built_lib):
    """bilinear in = 32 * out passes and 32 * out + 1 does not; bicubic passes at 16 x; Lanczos passes at 3 * in = 32 * out -- per axis"""
    def ok(filter, in_w, in_h, w, h):
        arr = _images(w=max(in_w, 1), h=max(in_h, 1), num_chans=3)
        return _plan(arr=arr, r=_rend(filter=fpng_amd.RENDITION_FILTERS[filter], w=w, h=h, out_cap=1 << 24)) == 0
    for f, lim in (("bilinear", 32), ("nearest", 32), ("box", 32), ("hamming", 32), ("bicubic", 16)):
        for out in (1, 3, 65):
            assert ok(f, lim * out, 7, out, 7) and ok(f, 7, lim * out, 7, out), (f, out)
            assert not ok(f, lim * out + 1, 7, out, 7) and not ok(f, 7, lim * out + 1, 7, out), (f, out)
    for i, o in ((32, 3), (704, 66), (2048, 192)):
        assert 3 * i == 32 * o and ok("lanczos", i, 9, o, 9) and ok("lanczos", 9, i, 9, o)
        assert not ok("lanczos", i + 1, 9, o, 9) and not ok("lanczos", 9, i + 1, 9, o)
    # the limit is the BOX's, not the image's
    arr = _images(w=4000, h=3000, num_chans=3)
    assert _plan(arr=arr, r=_rend(box_x=1, box_y=1, box_w=640, box_h=320, w=20, h=10, out_cap=1 << 20)) == 0
    assert _plan(arr=arr, r=_rend(box_x=1, box_y=1, box_w=641, box_h=320, w=20, h=10, out_cap=1 << 20)) == INVALID_ARG


def test_the_scratch_offsets_are_aligned_and_do_not_overlap(built_lib):
    rng = np.random.default_rng(3)
    imgs = (_lib.Image * 2)()
    for a, c in zip(imgs, (3, 4)):
        a.d_pixels, a.w, a.h, a.num_chans = 0x10000, 300, 200, c
    n = 40
    r = (_lib.Rendition * n)()
    for k in range(n):
        r[k].image, r[k].filter = k & 1, k % 6
        r[k].w, r[k].h = (5, 3) if k == 0 else (int(rng.integers(100, 400)), int(rng.integers(70, 300)))
    r[0].box_w, r[0].box_h = 40, 24  # (5 x 3 within every filter's limit)
    rc, total, offs = _plan(arr=imgs, n_images=2, r=r, n=n, packed=1, want_offsets=True)
    assert rc == 0 and offs[0] == 0 and offs[1] == 48  # (5 x 3 RGB is 45 bytes: the RGBA rendition behind it begins at the next 16)
    end = 0
    for k in range(n):
        assert offs[k] % 16 == 0 and end <= offs[k] < end + 16, k
        end = offs[k] + r[k].w * r[k].h * (3 + (k & 1))
    assert total >= end + 16 and total % 16 == 0  # room behind the last one for the row walk's aligned reads


# ---- the Python door ----
def test_rendition_records_and_the_plan_through_python(built_lib):
    r = fpng_amd.rendition(3, (20, 10), (1, 2, 30, 40), "lanczos", "premultiplied")
    assert (r.image, r.filter, r.box_x, r.box_y, r.box_w, r.box_h, r.w, r.h, r.alpha_op, r.reserved, r.d_out, r.out_cap) == (3, 5, 1, 2, 30, 40, 20, 10, 2, 0, None, 0)
    r = fpng_amd.rendition(0, (7, 9))
    assert (r.filter, r.box_x, r.box_y, r.box_w, r.box_h, r.alpha_op) == (0, 0, 0, 0, 0, 0)
    for bad in (dict(filter="cubic"), dict(alpha="composite"), dict(size=(-1, 5)), dict(box=(0, 0, 1 << 32, 1))):
        with pytest.raises(ValueError):
            fpng_amd.rendition(**dict(dict(image=0, size=(4, 4)), **bad))
    t = torch.zeros((40, 64, 3), dtype=torch.uint8)
    total, offs = fpng_amd.renditions_plan([t], [fpng_amd.rendition(0, (5, 3)), fpng_amd.rendition(0, (20, 10), (1, 1, 60, 30), "bicubic")], packed=True)
    assert offs == [0, 48] and total >= 48 + 600
    with pytest.raises(fpng_amd.FpngAmdError) as e:
        fpng_amd.renditions_plan([t], [fpng_amd.rendition(0, (1, 1))], packed=True)
    assert e.value.code == INVALID_ARG
    with pytest.raises(fpng_amd.FpngAmdError):  # (without a pack a rendition needs its d_out)
        fpng_amd.renditions_plan([t], [fpng_amd.rendition(0, (5, 3))])
    with pytest.raises(ValueError):
        fpng_amd.renditions_plan([t], [fpng_amd.rendition(0, (5, 3))], kind="hwc")
    with pytest.raises(fpng_amd.FpngAmdError) as e:
        fpng_amd.rendition_pixels(t, fpng_amd.rendition(1, (5, 3)))
    assert e.value.code == INVALID_ARG


# ---- the documentation's examples ----
def test_documented_examples_pass_the_validation(built_lib):
    """INTEGRATION.md's examples of the renditions call, record by record as the text has them, through the submit call's validation:
    an example beyond a filter's scale limit is one the library refuses"""
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "INTEGRATION.md")) as f:
        text = f.read()
    sec = text[text.index("### Resized renditions of device images"):]
    sec = sec[:sec.index("\n## ")]
    # Python: enc.encode_renditions([source], [records], kind=...) over the sources whose shapes the text's comments state
    assert "(4320, 7680, 4) uint8" in sec and "float16 (3, 1024, 1024)" in sec
    sources = {"frame": torch.empty((4320, 7680, 4), dtype=torch.uint8), "chw": torch.empty((3, 1024, 1024), dtype=torch.float16)}
    calls = re.findall(r"enc\.encode_renditions\(\[(\w+)\], \[(.*?)\](?:, kind=\"(\w+)\")?\)", sec, re.S)
    assert sorted(c[0] for c in calls) == ["chw", "frame"]
    for name, records, kind in calls:
        rends = eval("[" + records + "]", {"fpng_amd": fpng_amd})
        assert len(rends) == 2
        total, offs = fpng_amd.renditions_plan([sources[name]], rends, kind=kind or "image", packed=True)
        assert total > 0 and len(offs) == 2, name
    # C: the initialisers of fpng_amd_rendition r[2], over the frame the comment above them states
    assert "frame: a 3840 x 2160 RGBA fpng_amd_image" in sec
    rows = re.findall(r"\{(?:/\*image\*/ )?(\d+), FPNG_AMD_RENDITION_(\w+), (\d+), (\d+), (\d+), (\d+), (?:/\*w, h\*/ )?(\d+), (\d+), (\w+), (\d+), d_\w+, \w+_cap\}", sec)
    assert len(rows) == 2
    rends = []
    for image, filter, bx, by, bw, bh, w, h, alpha, reserved in rows:
        assert alpha in ("0", "FPNG_AMD_ALPHA_PREMULTIPLIED") and reserved == "0"
        box = tuple(int(v) for v in (bx, by, bw, bh))
        rends.append(fpng_amd.rendition(int(image), (int(w), int(h)), box if any(box) else None, filter.lower(), "premultiplied" if alpha != "0" else None))
    fpng_amd.renditions_plan([torch.empty((2160, 3840, 4), dtype=torch.uint8)], rends, packed=True)
