"""GPU tests (-m gpu) of fpng_amd_encode_submit_renditions: resized copies of device images, resampled by enc_resize_kernel from the
source as it lies and encoded by the unchanged chain.  The bar for the pixels is rendition_model.pixels (the existing Python models,
pinned to Pillow in test_renditions_cpu.py), for the files test_gpu_layouts._expect (the reference, or the pinned oracle) of those
pixels, byte for byte, in flags 0, 1 and 2; for a packed call's placement fpng_amd.pack_place on the reference's sizes and the
arena's prefill.  Nothing expected comes from the library."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import alpha_model as AM
import rendition_model as RM
from test_float_encode_cpu import IMAGENET_MEAN, IMAGENET_STD, float_image
from rendition_cases import ex_view, float_tensor, planar_view
from test_gpu_layouts import _expect, _same
from test_gpu_packed import _arena, _check, _need

pytestmark = pytest.mark.gpu

FLAGS = [0, 1, 2]
INVALID_ARG, BUFFER_TOO_SMALL, ARENA_FULL = -1, -4, 2
TILE_SIZES = [(1, 1), (63, 15), (64, 16), (65, 17), (130, 33)]  # around the 64 x 16 tile, and more than one tile each way


@pytest.fixture(scope="module")
def enc(built_lib):
    import torch
    import fpng_amd
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    e = fpng_amd.Encoder(device=0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def expected():
    """the judge's file for (pixels, flags), made once per distinct image"""
    made = {}

    def get(img, flags):
        key = (img.shape, img.tobytes(), flags)
        if key not in made:
            made[key] = _expect(img, flags)
        return made[key]
    return get


def _noise(w, h, c, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, c), dtype=np.uint8)


_PIXELS = {}


def _pixels(img, spec):
    """the model's pixels of rendition spec = (image, size, box, filter, alpha) of img, made once per image CONTENT and spec"""
    key = (img.shape, hashlib.sha1(img.tobytes()).digest()) + tuple(spec[1:])
    if key not in _PIXELS:
        _PIXELS[key] = RM.pixels(img, spec[1], spec[2], spec[3], spec[4])
    return _PIXELS[key]


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _judge(pngs, names, imgs, specs, flags, expected, what):
    assert len(pngs) == len(specs)
    for k, (png, s) in enumerate(zip(pngs, specs)):
        _same(png, expected(_pixels(imgs[s[0]], s), flags), f"{what}: {names[s[0]]}, rendition {k} {s[1:]} flags {flags}")


def _encode(enc, tensors, specs, flags, kind="image", **layout):
    import fpng_amd
    return enc.encode_renditions(tensors, [fpng_amd.rendition(*s) for s in specs], kind=kind, flags=flags, **layout)


# ---- sources in the layouts of the four descriptor kinds (rendition_cases.py), on the GPU ----
def _ex_view(img, name, pitch_kind, fill):
    return ex_view(img, name, pitch_kind, fill, "cuda")


def _planar_view(img, reverse, fill):
    return planar_view(img, reverse, fill, "cuda")


def _unchanged(keep):
    for d, host in keep:
        assert np.array_equal(d.cpu().numpy(), host), "the call wrote into a source buffer"


# ---- tile edges ----
@pytest.fixture(scope="module")
def tile_cases():
    return _tile_cases()


def _tile_cases():
    """(names, images, specs): every filter to every tile size from a 600 x 130 noise image (non-integer ratios; 1 x 1 from a box
    within the scale limits) and from 2 x 2 and 1 x 1 images (growing), RGB and RGBA"""
    names, imgs, specs = [], [], []
    for c in (3, 4):
        for (w, h) in [(600, 130), (2, 2), (1, 1)]:
            names.append(f"tile{w}x{h}x{c}")
            imgs.append(_noise(w, h, c, 10 * w + c))
            i = len(imgs) - 1
            for f in RM.FILTERS:
                for size in TILE_SIZES:
                    box = (7, 3, 10, 9) if (w, size) == (600, (1, 1)) else None
                    specs.append((i, size, box, f, "premultiplied" if c == 4 and f in ("bicubic", "box") else None))
    return names, imgs, specs


@pytest.mark.parametrize("flags", FLAGS)
def test_tile_edges(enc, expected, tile_cases, flags):
    names, imgs, specs = tile_cases
    for c in (3, 4):  # (a call's images share a kind: "image" takes both channel counts)
        pick = [s for s in specs if imgs[s[0]].shape[2] == c]
        _judge(_encode(enc, [_cuda(im) for im in imgs], pick, flags), names, imgs, pick, flags, expected, f"tile edges, {c} channels")


# ---- scale limits: the widest taps and the most tile rows (the LDS bound) ----
@pytest.mark.parametrize("flags", FLAGS)
def test_scale_limits(enc, expected, flags):
    img = _noise(2080, 544, 4, 77)
    rgb = np.ascontiguousarray(img[..., :3])
    specs = [(0, (65, 17), None, "bilinear", None),                   # 2080 x 544 -> 65 x 17: 32 x
             (0, (65, 17), (517, 135, 1040, 272), "bicubic", None),   # 1040 x 272 -> 65 x 17: 16 x
             (0, (66, 3), (3, 500, 704, 32), "lanczos", None),        # 704 wide -> 66, 32 rows -> 3: 3 * in = 32 * out
             (0, (65, 17), None, "box", None), (0, (65, 17), None, "hamming", None), (0, (65, 17), None, "nearest", None),
             (0, (65, 17), None, "bilinear", "premultiplied")]
    _judge(_encode(enc, [_cuda(img)], specs, flags), ["limit4"], [img], specs, flags, expected, "scale limits, RGBA")
    _judge(_encode(enc, [_cuda(rgb)], specs[:6], flags), ["limit3"], [rgb], specs[:6], flags, expected, "scale limits, RGB")


# ---- the threshold between the fused horizontal pass and the channels taking turns (encode_resize.h: enc_resize_fused) ----
def test_both_sides_of_the_fused_pass(enc, expected):
    """a 4-byte source's tile holds T once per channel up to 32 KB of LDS: with 64 columns kept and 17 rows made of 100 .. 120, a row
    more at a time, that bound is crossed between 6 x and 7 x (29.4 KB at 102 rows, 33.9 KB at 119)"""
    img = _noise(64, 120, 4, 90)
    specs = [(0, (64, 17), (0, 0, 64, in_h), "bilinear", "premultiplied" if in_h & 1 else None) for in_h in range(100, 121)]
    _judge(_encode(enc, [_cuda(img)], specs, 0), ["fused"], [img], specs, 0, expected, "fused threshold")


# ---- boxes ----
@pytest.mark.parametrize("flags", FLAGS)
def test_boxes(enc, expected, flags):
    """a box at (1, 1) of a 3-byte source with an odd pitch and an odd start byte, one touching the right and bottom edges, the whole"""
    img = _noise(76, 41, 3, 5)
    d, host, view, order, up = _ex_view(img, "BGR", "odd", np.random.default_rng(6))
    assert view.data_ptr() % 2 == 1 and view.stride(0) % 2 == 1
    specs = [(0, (33, 17), (1, 1, 50, 30), f, None) for f in ("bilinear", "lanczos")] + [(0, (20, 30), (41, 11, 35, 30), f, None) for f in ("bicubic", "nearest")] + \
            [(0, (64, 16), None, "hamming", None), (0, (76, 41), (0, 0, 76, 41), "box", None)]
    _judge(_encode(enc, [view], specs, flags, kind="ex", order=order, bottom_up=up), ["box3"], [img], specs, flags, expected, "boxes")
    _unchanged([(d, host)])


# ---- layouts: every descriptor kind ----
LAYOUT_SPECS = [(0, (65, 17), None, "bilinear", None), (0, (31, 33), (2, 3, 90, 40), "bicubic", None), (0, (9, 5), (60, 20, 9, 5), "nearest", None)]


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("name,pitch_kind", [("BGR", "wide"), ("BGRA", "packed"), ("ARGB", "neg"), ("XRGB", "neg"), ("RGBX", "wide"), ("ABGR", "wide")])
def test_layouts_interleaved(enc, expected, name, pitch_kind, flags):
    import fpng_amd
    c = fpng_amd.SRC_FORMATS[name][2]
    img = _noise(97, 45, c, 20 + c)
    d, host, view, order, up = _ex_view(img, name, pitch_kind, np.random.default_rng(8))
    specs = LAYOUT_SPECS + ([(0, (40, 20), None, "hamming", "premultiplied")] if c == 4 else [])
    _judge(_encode(enc, [view], specs, flags, kind="ex", order=order, bottom_up=up), [f"lay{c}"], [img], specs, flags, expected, f"{name} {pitch_kind}")
    _unchanged([(d, host)])


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("c", [3, 4])
@pytest.mark.parametrize("reverse", [False, True])
def test_layouts_planar(enc, expected, reverse, c, flags):
    img = _noise(97, 45, c, 20 + c)
    d, host, view, order = _planar_view(img, reverse, np.random.default_rng(9))
    specs = LAYOUT_SPECS + ([(0, (40, 20), None, "box", "premultiplied")] if c == 4 else [])
    _judge(_encode(enc, [view], specs, flags, kind="planar", order=order), [f"lay{c}"], [img], specs, flags, expected, f"planar reverse {reverse}")
    _unchanged([(d, host)])


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("code", [0, 1, 2])
def test_layouts_float(enc, expected, code, flags):
    """f32, f16 and bf16 planes under the inverse of Normalize(mean, std): the rendition is the resize of the quantised bytes"""
    import fpng_amd
    c = 3 + (code & 1)
    scale, bias = fpng_amd.denormalize_constants(IMAGENET_MEAN, IMAGENET_STD)
    base = _noise(97, 45, c, 30 + code)
    el, img = float_image(base, code, scale, bias, np.random.default_rng(40 + code),
                          to_float=lambda u, ch: (u - IMAGENET_MEAN[ch]) / IMAGENET_STD[ch] if ch < 3 else u)
    specs = LAYOUT_SPECS + ([(0, (40, 20), None, "bilinear", "premultiplied")] if c == 4 else [])
    pngs = _encode(enc, [float_tensor(el, code, "cuda")], specs, flags, kind="float", mean=IMAGENET_MEAN, std=IMAGENET_STD)
    _judge(pngs, [f"float{code}"], [img], specs, flags, expected, f"float code {code}")


# ---- nothing outside the box's pixels matters ----
@pytest.mark.parametrize("flags", [0, 2])
def test_no_influence_from_outside(enc, expected, flags):
    """two runs whose pitch padding, X bytes, fourth plane and pixels outside the box differ: the same files, the model's"""
    box = (11, 7, 60, 30)
    inside = _noise(97, 45, 3, 50)
    specs = [(0, (33, 17), box, f, None) for f in ("bilinear", "bicubic", "nearest", "lanczos")] + [(0, (60, 30), box, "box", None)]
    runs = []
    for seed in (1, 2):
        fill = np.random.default_rng(100 + seed)
        img = fill.integers(0, 256, inside.shape, dtype=np.uint8)
        img[box[1]:box[1] + box[3], box[0]:box[0] + box[2]] = inside[box[1]:box[1] + box[3], box[0]:box[0] + box[2]]
        d, host, view, order, up = _ex_view(img, "XBGR", "wide", fill)
        ex = _encode(enc, [view], specs, flags, kind="ex", order=order, bottom_up=up)
        d2, host2, pview, porder = _planar_view(img, False, fill)
        pl = _encode(enc, [pview], specs, flags, kind="planar", order=porder)
        _unchanged([(d, host), (d2, host2)])
        runs.append(ex + pl)
    assert runs[0] == runs[1], "bytes outside the box's pixels changed a file"
    _judge(runs[0], ["inside"], [inside], specs + specs, flags, expected, "no influence")


# ---- alpha ----
@pytest.mark.parametrize("flags", FLAGS)
def test_alpha(enc, expected, flags):
    """premultiplied against straight on alpha_model's pattern (transparent next to opaque bright samples: U's clip is live), and
    the identity rendition, which is a copy whatever the op"""
    img = AM.pattern(83, 61, seed=3)
    specs = []
    for f in RM.FILTERS:
        specs += [(0, (40, 29), None, f, a) for a in (None, "premultiplied")]
        specs.append((0, (30, 20), (5, 6, 30, 20), f, "premultiplied"))  # size == box: a copy
        specs.append((0, (90, 70), (5, 6, 30, 20), f, "premultiplied"))  # growing
    pngs = _encode(enc, [_cuda(img)], specs, flags)
    _judge(pngs, ["alpha"], [img], specs, flags, expected, "alpha")
    differ = sum(1 for f in RM.FILTERS if f != "nearest" and not np.array_equal(_pixels(img, (0, (40, 29), None, f, None)),
                                                                                  _pixels(img, (0, (40, 29), None, f, "premultiplied"))))
    assert differ == 5, "the two alpha rules must differ on this image for every convolution filter"
    assert np.array_equal(_pixels(img, (0, (30, 20), (5, 6, 30, 20), "bicubic", "premultiplied")), img[6:26, 5:35])


# ---- one call that mixes images, channel counts, filters and sizes; one rendition alone ----
@pytest.mark.parametrize("flags", FLAGS)
def test_mixed_call_and_a_single_rendition(enc, expected, flags):
    import fpng_amd
    imgs = [_noise(120, 50, 3, 60), AM.pattern(77, 66, seed=4)]
    names = ["mixed3", "mixed4"]
    # planar takes 3 and 4 planes in one call; the first rendition is 5 x 3 RGB (45 bytes), so the RGBA one behind it begins at 48
    views = [_planar_view(im, False, None)[2] for im in imgs]
    specs = [(0, (5, 3), None, "bilinear", None), (1, (37, 21), None, "bicubic", "premultiplied"), (0, (121, 51), None, "lanczos", None),
             (1, (9, 9), (60, 50, 9, 9), "nearest", None), (1, (150, 17), (1, 2, 75, 60), "hamming", None)]
    _, offs = fpng_amd.renditions_plan(views, [fpng_amd.rendition(*s) for s in specs], kind="planar", packed=True)
    assert offs[:2] == [0, 48]
    _judge(_encode(enc, views, specs, flags, kind="planar"), names, imgs, specs, flags, expected, "mixed call")
    for s in (specs[1], specs[2]):  # one rendition: its job record travels in the chain's first kernel's arguments
        _judge(_encode(enc, views, [s], flags, kind="planar"), names, imgs, [s], flags, expected, "a single rendition")


# ---- packed ----
@pytest.mark.parametrize("flags", [0, 1])
def test_packed(enc, expected, flags):
    """offsets and statuses are fpng_amd.pack_place's on the reference's sizes, arena bytes outside the extents keep their prefill,
    a full arena refuses per file"""
    import torch
    import fpng_amd
    imgs = [_noise(120, 50, 3, 60), _noise(90, 70, 3, 61)]
    names = ["mixed3", "packed3"]
    specs = [(0, (64, 16), None, "bilinear", None), (1, (30, 30), None, "bicubic", None), (0, (5, 3), None, "box", None), (1, (100, 80), None, "hamming", None),
             (0, (17, 9), (3, 3, 100, 40), "lanczos", None), (1, (1, 1), (4, 4, 2, 2), "nearest", None)]
    files = [expected(_pixels(imgs[s[0]], s), flags) for s in specs]
    sizes = [len(f) for f in files]
    n = len(specs)
    rends = [fpng_amd.rendition(*s) for s in specs]
    tensors = [_cuda(im) for im in imgs]
    for align, lead in [(16, 0), (512, 512)]:
        need = _need(sizes, align, lead)
        full = fpng_amd.pack_capacity([(s[1][0], s[1][1], 3) for s in specs], align, lead)
        for cap, refused in [(full, 0), (need, 0), (need - 1, 1), (_need(sizes, align, lead, 2), n - 2), (16, n)]:
            arena, pat = _arena(max(full, cap), align)
            table = torch.full((2 * (n + 1),), -1, dtype=torch.int64, device="cuda")
            assert enc.submit_renditions(tensors, rends, arena=arena[:cap], align=align, lead=lead, table=table, flags=flags) == n
            recs, total = enc.wait_packed(enc.last_ticket, n)
            what = f"packed renditions, arena of {cap} (need {need}) align {align} flags {flags}"
            _check(arena, pat, recs, total, files, sizes, align, lead, cap, what)
            assert [st for _, _, _, st in recs] == [0] * (n - refused) + [ARENA_FULL] * refused, what
            t = table.cpu().numpy().reshape(n + 1, 2)
            assert [tuple(r) for r in t[:n]] == [(off, size) for off, size, _, _ in recs], f"{what}: d_table differs from the host records"
            assert [(size, st) for _, size, _, st in recs] == enc_wait_sizes(enc, n), what


def enc_wait_sizes(enc, n):
    """the packed ticket through fpng_amd_encode_wait: sizes without offsets"""
    return [(size, st) for size, _, st in enc.wait(enc.last_ticket, n)]


# ---- lanes ----
def test_lanes_and_a_growing_scratch(built_lib, expected):
    """2 * lanes + 1 submissions without a wait between them on a fresh encoder: a lane's second submission is larger than its first,
    the last one larger still, so a lane's scratch grows while its earlier submission may still run; then all are collected and judged.
    A ticket's records live for RING = 8 submissions, so with four lanes and more the ticket RING back is collected in front of a
    submission -- the one wait the interface itself demands; the submissions are 2 * lanes + 1 whatever the lanes."""
    import torch
    import fpng_amd
    RING = 8
    enc = fpng_amd.Encoder(device=0)
    try:
        lanes = enc.lanes
        n_sub = 2 * lanes + 1
        img = _noise(600, 130, 4, 70)
        t = _cuda(img)
        sizes = [(5, 3)] * lanes + [(400, 300)] * lanes + [(700, 500)]
        filters = ["bilinear", "bicubic", "box", "nearest", "hamming"]
        subs, results = [], {}
        for i in range(n_sub):
            if i >= RING:
                results[i - RING] = enc.wait(subs[i - RING][0], len(subs[i - RING][1]))
            size = sizes[i]
            specs = [(0, size, (10, 10, 60, 36) if size == (5, 3) else None, filters[i % 5], None), (0, (33, 9), (i, i, 300, 100), "bilinear", "premultiplied")]
            outs = [torch.empty(fpng_amd.max_encoded_size(s[1][0], s[1][1], 4) + 64, dtype=torch.uint8, device="cuda") for s in specs]
            enc.submit_renditions([t], [fpng_amd.rendition(*s) for s in specs], outs=outs, flags=i % 2)
            subs.append((enc.last_ticket, specs, outs, i % 2))
        assert len(subs) == 2 * lanes + 1
        for i, (ticket, specs, outs, flags) in enumerate(subs):
            res = results[i] if i in results else enc.wait(ticket, len(specs))
            assert all(st == 0 for _, _, st in res)
            pngs = [bytes(o[:size].cpu().numpy()) for o, (size, _, _) in zip(outs, res)]
            _judge(pngs, ["lanes"], [img], specs, flags, expected, f"ticket {ticket}")
        assert np.array_equal(t.cpu().numpy(), img)
    finally:
        enc.close()


# ---- refusals ----
def _submit_raw(enc, kind, arr, n_images, fmt, rarr, n, flags, pack):
    t = C.c_uint64(0)
    enc._sync_stream()
    rc = enc.lib.fpng_amd_encode_submit_renditions(enc.h, kind, C.cast(arr, C.c_void_p) if arr is not None else None, n_images, C.byref(fmt) if fmt is not None else None,
                                                   rarr, n, flags, C.byref(pack) if pack is not None else None, C.byref(t))
    return rc, t.value


def test_refusals(enc, expected):
    """every refusal of the header: the return code, no ticket, the sources as they were, and a valid submission right behind"""
    import torch
    import fpng_amd
    from fpng_amd import _lib
    img = _noise(64, 40, 4, 80)
    t = _cuda(img)
    out = torch.empty(fpng_amd.max_encoded_size(64, 40, 4) + 64, dtype=torch.uint8, device="cuda")
    arena, _ = _arena(1 << 16, 16)
    before = enc.last_ticket if hasattr(enc, "last_ticket") else 0

    def images(**kw):
        arr = (_lib.Image * 1)()
        arr[0].d_pixels, arr[0].w, arr[0].h, arr[0].num_chans = t.data_ptr(), 64, 40, 4
        for k, v in kw.items():
            setattr(arr[0], k, v)
        return arr

    def rend(**kw):
        arr = (_lib.Rendition * 1)()
        r = arr[0]
        r.image, r.filter, r.w, r.h, r.d_out, r.out_cap = 0, 0, 20, 10, out.data_ptr(), out.numel()
        for k, v in kw.items():
            setattr(r, k, v)
        return arr

    pack = _lib.Pack(arena.data_ptr(), arena.numel(), 16, 0, None, 0)
    fmt = _lib.FloatFormat()
    bad = [("unknown kind", INVALID_ARG, dict(kind=4)), ("unknown filter", INVALID_ARG, dict(r=rend(filter=6))), ("unknown alpha op", INVALID_ARG, dict(r=rend(alpha_op=3))),
           ("the composite op", INVALID_ARG, dict(r=rend(alpha_op=1))), ("image >= n_images", INVALID_ARG, dict(r=rend(image=1))),
           ("box partly zero", INVALID_ARG, dict(r=rend(box_x=1, box_y=1, box_w=0, box_h=5))), ("box empty", INVALID_ARG, dict(r=rend(box_w=5))),
           ("box outside, x", INVALID_ARG, dict(r=rend(box_x=60, box_w=5, box_h=5))), ("box outside, y", INVALID_ARG, dict(r=rend(box_y=36, box_w=5, box_h=5))),
           ("box outside, wrap", INVALID_ARG, dict(r=rend(box_x=0xFFFFFFFF, box_w=2, box_h=2))),
           ("w = 0", INVALID_ARG, dict(r=rend(w=0))), ("h past 2^24", INVALID_ARG, dict(r=rend(h=(1 << 24) + 1))),
           ("scale, bilinear", INVALID_ARG, dict(r=rend(w=1))), ("scale, bicubic", INVALID_ARG, dict(r=rend(filter=1, w=3))), ("scale, lanczos", INVALID_ARG, dict(r=rend(filter=5, w=5))),
           ("reserved", INVALID_ARG, dict(r=rend(reserved=1))), ("no renditions", INVALID_ARG, dict(n=0)), ("65536 renditions", INVALID_ARG, dict(n=65536)),
           ("d_out with a pack", INVALID_ARG, dict(pack=pack)), ("no d_out without a pack", INVALID_ARG, dict(r=rend(d_out=None, out_cap=0))),
           ("d_out misaligned", INVALID_ARG, dict(r=rend(d_out=out.data_ptr() + 8))), ("out_cap", BUFFER_TOO_SMALL, dict(r=rend(out_cap=fpng_amd.max_encoded_size(20, 10, 4) - 1))),
           ("an image's d_out", INVALID_ARG, dict(arr=images(d_out=out.data_ptr(), out_cap=out.numel()))), ("an image's out_cap", INVALID_ARG, dict(arr=images(out_cap=1))),
           ("fmt with kind image", INVALID_ARG, dict(fmt=fmt)), ("no images", INVALID_ARG, dict(n_images=0)),
           ("a bad pack", INVALID_ARG, dict(pack=_lib.Pack(arena.data_ptr(), arena.numel(), 24, 0, None, 0), r=rend(d_out=None, out_cap=0)))]
    spec = (0, (20, 10), None, "bilinear", None)
    want = expected(_pixels(img, spec), 0)
    for what, code, kw in bad:
        rc, ticket = _submit_raw(enc, kw.get("kind", 0), kw.get("arr", images()), kw.get("n_images", 1), kw.get("fmt"), kw.get("r", rend()), kw.get("n", 1), 0, kw.get("pack"))
        assert (rc, ticket) == (code, 0), f"{what}: rc {rc} ticket {ticket}"
        # the same records through the plan function, where it sees them (it takes no pack and no encoder)
        if what != "a bad pack":
            rc2 = enc.lib.fpng_amd_renditions_plan(kw.get("kind", 0), C.cast(kw.get("arr", images()), C.c_void_p), kw.get("n_images", 1), C.byref(kw["fmt"]) if "fmt" in kw else None,
                                                   kw.get("r", rend()), kw.get("n", 1), 1 if "pack" in kw else 0, None, None)
            assert rc2 == code, f"{what}: the plan says {rc2}"
        rc, ticket = _submit_raw(enc, 0, images(), 1, None, rend(), 1, 0, None)
        assert rc == 0 and ticket == before + 1, f"after {what}: rc {rc}, ticket {ticket} behind {before}"
        before = ticket
        (size, _, status), = enc.wait(ticket, 1)
        assert status == 0
        _same(bytes(out[:size].cpu().numpy()), want, f"the submission behind the refusal of {what}")
    assert np.array_equal(t.cpu().numpy(), img)
