"""GPU decoder of several resized views of each file THROUGH A PER-VIEW TONE RECORD (-m gpu;
fpng_amd_decode_batch(_device)_planar_views_tone and _hwc_views_tone: the warp call, and for a view with an op
dec_view_tone_hist_kernel's histograms of the un-mirrored uint8 window in the scratch -- through the warp's gather where there is
one, fill samples included -- dec_view_tone_lut_kernel's tables, and dec_view_post_kernel's look-up wherever it loads a sample, the
blur's reflected halo included): autocontrast, equalize and contrast; planar and channels-last destinations, uint8 and the three
float dtypes, three and four channels, mirrors, host and device files, with warps of both filters, blurs, point operations and
matrices; tone, post-only and direct views mixed in one file.

Expected values never come from the library: the bytes are the REFERENCE's decoder's, resized by resize_view_model.py, coloured by
color_model.py, warped by warp_model.py, toned by tone_model.py and post-processed by post_model.py (exact restatements;
test_views_tone_cpu.py holds tone_model against the host twins and Pillow).  The guarantee tests alone compare calls of the library
with each other, as the guarantees say.  Every call decodes into ONE sentinel-filled buffer that is compared WHOLE and bit for bit.

A tone record here is tone_model's dict: {"autocontrast": True}, {"equalize": True} or {"contrast": factor}, {} for a view without an
op; warp and post records are warp_model's and post_model's dicts."""
import numpy as np
import pytest

from test_gpu_decode import UNDECIDED, _device_files
from test_gpu_decode_float import CONSTS
from test_gpu_decode_layouts import SENTINEL, _damaged_files, _header_dims
from test_gpu_decode_planar import KINDS as PLANAR_KINDS, _Region as _PlanarRegion
from test_gpu_decode_resize import BITS, DTYPES, ELEM, _encode_gpu, _Files, enc, files  # noqa: F401  (enc, files: fixtures)
from test_gpu_decode_views_color import LAYOUTS, _difference, _matrices
from test_gpu_decode_views_hwc import KINDS as HWC_KINDS, _Region as _HwcRegion
from test_gpu_decode_views_post import _records as _post_records
from test_gpu_decode_views_warp import W3, W64, W65, W130, _decode as _warp_decode, _matrix, _warp_plan, _warp_records
from test_gpu_resize_view import _Model, _window, model  # noqa: F401  (model: a fixture)
import resize_view_model as VM
import tone_model as TM

pytestmark = pytest.mark.gpu

AUTO, EQUAL = {"autocontrast": True}, {"equalize": True}


def _tone_records(tone):
    import fpng_amd
    return [[fpng_amd.view_tone(**p) for p in ps] for ps in tone]


def _decode(enc, layout, pngs, plan, dtype, device, color, post, warp, tone, dev=None, consts=CONSTS[0]):  # noqa: F811
    """test_gpu_decode_views_warp's _decode with tone= (per file a list of a tone record per view; post, warp None: no post=, warp= at
    all): ONE call into ONE sentinel-filled buffer -> (results, the buffer afterwards, the tensors, the regions in the records' order)"""
    import torch
    e = ELEM[dtype]
    regs, off = [], 0
    for c, views in plan:
        for _, full, window, _, _, kind in views:
            w, h = _window(full, window)[2:]
            r = _PlanarRegion(off, w, h, c, kind) if layout == "planar" else _HwcRegion(off, w, h, c, kind, e)
            regs.append(r)
            off += r.size
    buf = torch.full((off * e if layout == "planar" else off,), SENTINEL, dtype=torch.uint8, device="cuda")
    typed = buf.view(getattr(torch, dtype))
    it = iter(regs)
    per = [[next(it) for _ in views] for _, views in plan]
    if layout == "planar":
        outs = [[typed.as_strided((r.c, r.h, r.w), (r.pp, r.rp, 1), r.lo) for r in rs] for rs in per]
    else:
        outs = [[r.view(typed) for r in rs] for rs in per]
    kw = {} if dtype == "uint8" else {"scale": consts[0], "bias": consts[1]}
    args = ([[v[0] for v in views] for _, views in plan], outs, [[v[1] for v in views] for _, views in plan], [[v[2] for v in views] for _, views in plan],
            [[v[3] for v in views] for _, views in plan])
    kw.update(mirror=[[v[4] for v in views] for _, views in plan], order=[[r.order() for r in rs] for rs in per], bottom_up=[[r.kind == "bottom_up" for r in rs] for rs in per])
    kw["tone"] = _tone_records(tone)
    if warp is not None:
        kw["warp"] = _warp_records(warp)
    if post is not None:
        kw["post"] = _post_records(post)
    if color is not None:
        kw["color"] = color
    if device:
        call = enc.decode_device_views if layout == "planar" else enc.decode_device_views_hwc
        got = call(dev if dev is not None else _device_files(pngs, shift=1), *args, **kw)
    else:
        call = enc.decode_batch_views if layout == "planar" else enc.decode_batch_views_hwc
        got = call(pngs, *args, **kw)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    return got, (host.view(BITS[e]) if layout == "planar" else host), outs, regs


def _sources(model, idx, plan, dtype, color, post, warp, tone, skip=(), consts=CONSTS[0]):  # noqa: F811
    """the (oh, ow, c) element bits of every view under its matrix (color None: the identity), warp (None: none), tone and post
    record (None: no flags), in the records' order (None for the views of the files in `skip`)"""
    return [None if n in skip else TM.view_elements(model.view(idx[n], crop, full, window, f), c, dtype, m, None if color is None else color[n][k], consts,
                                                    {} if post is None else post[n][k], {} if warp is None else warp[n][k], tone[n][k])
            for n, (c, views) in enumerate(plan) for k, (crop, full, window, f, m, _) in enumerate(views)]


def _run(enc, files, model, layout, idx, plan, dtype, device, color, post, warp, tone, **kw):  # noqa: F811
    got, host, outs, regs = _decode(enc, layout, [files.pngs[i] for i in idx], plan, dtype, device, color, post, warp, tone, **kw)
    assert len(got) == len(idx)
    for n, (i, (st, views, cf)) in enumerate(zip(idx, got)):
        assert st == 0 and cf == files.chans[i] and len(views) == len(outs[n]) and all(a is b for a, b in zip(views, outs[n])), (n, i, st, cf)
    diff = _difference(layout, host, dtype, regs, _sources(model, idx, plan, dtype, color, post, warp, tone, consts=kw.get("consts", CONSTS[0])))
    assert diff is None, (layout, dtype, device, diff)


SOLID = np.array([[0, 0, 0, 77], [0, 0, 0, 0], [0, 0, 0, 255]], dtype=np.float32)  # (zeroes the input: the constant column alone)
TWO = np.array([[250, 0, 0, -28000], [0, 250, 0, -30000], [0, 0, 250, -25000]], dtype=np.float32)  # (a gain that leaves 0 and 255, and 250 at the one byte between)


def _tone_plan(files, layout, filter, k0):  # noqa: F811
    """counts 3, 15, 1: a 1 x 1 file under autocontrast or equalize (one bin: identity tables) and under contrast with a factor below
    and one above 1 (N = 1, a one-bin luma sum: mean = L of the one pixel, and a table that is not the identity), a 4-channel 600 x 130 file
    (k0 odd: the `noise` one) with fifteen views -- all three operations on every window (W3: equalize's step == 0; W64: one tile and
    one histogram workgroup; W65, W130: partial last tiles), alone, behind a warp of either filter that leaves fill inside the
    histogram, in front of a blur of R = 16 and R = 1 (the table applies to the halo's reflected samples), in front of solarize and
    posterize; a solid and a two-valued view through a matrix; a post-only view and a direct view between them -- and a 3-channel
    600 x 130 file at its own size (78000 samples: ten histogram workgroups whose atomics merge) whose fourth plane, when it has
    one, skips the stage.  k0 flips every mirror flag and swaps three and four channels.  -> idx, plan, color, post, warp, tone"""
    flip = bool(k0 & 1)
    kinds = PLANAR_KINDS if layout == "planar" else HWC_KINDS
    i600, whole, full = (5 if flip else 4), (0, 0, 600, 130), (300, 65)
    assert files.dims[i600] == (600, 130) and files.chans[i600] == 4 and files.dims[14 + flip] == (1, 1) and files.dims[2] == (600, 130) and files.chans[2] == 3
    near, lin = "nearest", "bilinear"
    big = (0, 0, 600, 130)  # (a window of the file at its own size: the full one)
    # (window, mirror, post, warp, tone, matrix or None: a seeded one)
    views = [(W130, False, {}, {}, AUTO, None),
             (W130, True, {"blur": (16, 5.0)}, {}, EQUAL, None),
             (W130, False, {}, {"a": _matrix(W130, angle=30.0), "filter": near, "fill": (10, 20, 30, 40)}, {"contrast": 1.6}, None),
             (W65, True, {"blur": (1, 0.5), "solarize": 100}, {"a": [1.0, 0.37, -2.5, 0.0, 1.0, 0.0], "filter": lin, "fill": (255, 0, 128, 7)}, EQUAL, None),
             (W65, False, {"solarize": 128, "posterize": 5}, {}, {"contrast": 0.4}, None),
             (W64, False, {}, {}, EQUAL, None),
             (W64, True, {"blur": (3, 1.0)}, {"a": _matrix(W64, angle=45.0), "filter": near, "fill": (1, 2, 3, 4)}, AUTO, None),
             (W3, False, {}, {}, EQUAL, None),
             (W3, True, {"blur": (1, 2.0)}, {}, {"contrast": 2.0}, None),
             (W130, False, {"blur": (11, 1.3), "posterize": 3}, {}, {}, None),
             (W65, True, {}, {}, {}, None),
             (W65, False, {}, {}, AUTO, SOLID),
             (W130, True, {"blur": (2, 1.0)}, {}, EQUAL, TWO),
             (W64, False, {}, {"a": _matrix(W64, angle=-10.0), "filter": lin, "fill": (9, 99, 199, 0)}, {"contrast": 1.5}, SOLID),
             (W65, True, {"posterize": 6}, {"a": _matrix(W65, angle=10.0, translate=(2.5, -1.25)), "filter": lin, "fill": (200, 100, 50, 25)}, AUTO, None)]
    idx = [14 + flip, i600, 2]
    ops = (AUTO, EQUAL, {"contrast": 0.5}, {"contrast": 3.0})
    plan = [(3 + flip, [((0, 0, 1, 1), (1, 1), None, filter, flip ^ bool(k & 1), kinds[(k0 + k) % len(kinds)]) for k in range(3)]),
            (4 - flip, [(whole, full, w, filter, m ^ flip, kinds[(k0 + k) % len(kinds)]) for k, (w, m, *_) in enumerate(views)]),
            (3 + flip, [(whole, (600, 130), big, filter, not flip, kinds[(k0 + 2) % len(kinds)])])]
    post = [[{}, {"solarize": 100}, {}], [v[2] for v in views], [{"blur": (16, 2.0)}]]
    warp = [[{}] * 3, [v[3] for v in views], [{}]]
    tone = [[ops[k0 % 2], ops[2], ops[3]], [v[4] for v in views], [ops[(k0 + 1) % 4]]]
    color = _matrices(plan, 300 + k0)
    for k, v in enumerate(views):
        if v[5] is not None:
            color[1][k] = v[5]
    assert [len(v) for _, v in plan] == [3, 15, 1]
    return idx, plan, color, post, warp, tone


# ---- 1. every element against the model ----
@pytest.mark.parametrize("dtype", ["uint8", "float"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_window_operation_warp_and_post_mixed_with_views_without_tone(enc, files, model, layout, dtype):  # noqa: F811
    """the batch of _tone_plan plain and flipped: uint8 and one float dtype per layout, bilinear and bicubic resizes, host and device
    files, dealt so that each value of each meets both values of the others"""
    dtype = "uint8" if dtype == "uint8" else ("float16" if layout == "planar" else "float32")
    d = (dtype != "uint8") + LAYOUTS.index(layout)
    for k0 in (0, 1):
        idx, plan, color, post, warp, tone = _tone_plan(files, layout, VM.FILTERS[(k0 + d) % 2], k0)
        if k0 == 0:  # (the plan does what its text says: a solid view, a two-valued one, fill inside a histogram, equalize's step == 0)
            c, views = plan[1]
            b = [TM.CM.element_bits_np(TM.CM.apply_np(color[1][k], np.ascontiguousarray(model.view(idx[1], *views[k][:4]).transpose(1, 2, 0))[..., :3]), "uint8") for k in (11, 12, 7)]
            assert all(len(np.unique(b[0][..., ch])) == 1 for ch in range(3)) and all(len(np.unique(b[1][..., ch])) <= 4 for ch in range(3))
            assert all(TM.equalize_entries(TM.histograms(b[2].transpose(2, 0, 1))[ch]) is None for ch in range(3))
            assert not TM.WM.apply_plane(warp[1][2], np.ones((33, 130), np.uint8), False, 0).all()
        for k in (1, 2):  # (the 1 x 1 file under contrast: the mean is the one pixel's L, and the table is not the identity)
            one = TM.CM.element_bits_np(TM.CM.apply_np(color[0][k], np.ascontiguousarray(model.view(idx[0], *plan[0][1][k][:4]).transpose(1, 2, 0))[..., :3]), "uint8").transpose(2, 0, 1)
            hist = TM.histograms(one)
            assert one.shape == (3, 1, 1) and hist[3].sum() == 1 and TM.contrast_mean(hist[3]) == int(TM.luma(one)[0, 0])
            assert "contrast" in tone[0][k] and not np.array_equal(TM.luts(tone[0][k], hist)[0], np.arange(256))
        _run(enc, files, model, layout, idx, plan, dtype, bool((k0 + d + d // 2) & 1), color, post, warp, tone, consts=CONSTS[k0])


@pytest.mark.parametrize("dtype", [t for t in DTYPES if t != "uint8"])
def test_the_other_dtypes_on_one_shape(enc, files, model, dtype):  # noqa: F811
    """every float dtype in both layouts on the 65 x 17 window: the three operations, mirrored and not, with and without posts and
    warps (NULL posts, warps and colours: the call's own records without flags)"""
    for layout in LAYOUTS:
        kinds = PLANAR_KINDS if layout == "planar" else HWC_KINDS
        whole, full = (0, 0, 600, 130), (300, 65)
        plan = [(4, [(whole, full, W65, "bilinear", bool(k & 1), kinds[k % len(kinds)]) for k in range(3)]), (4, [(whole, full, W65, "bicubic", True, kinds[-1])])]
        tone = [[AUTO, {"contrast": 1.25}, EQUAL], [{"contrast": 0.75}]]
        warp = [[{"a": _matrix(W65, angle=-15.0, shear=(8.0, 0.0)), "filter": "bilinear", "fill": (1, 128, 255, 64)}, {}, {}],
                [{"a": [1.0, 0.0, 3.0, 0.0, 1.0, -2.0], "filter": "nearest", "fill": (0, 255, 0, 255)}]]
        post = [[{"blur": (2, 1.0)}, {"posterize": 4}, {}], [{"solarize": 77}]]
        for with_others in (True, False):
            _run(enc, files, model, layout, [4, 2], plan, dtype, not with_others, _matrices(plan, 90) if with_others else None, post if with_others else None,
                 warp if with_others else None, tone)


def test_equalize_clips_its_table_on_the_gpu_too(enc):  # noqa: F811
    """the 380 x 202 image whose channels hold 0 x 1, 1 x 1000, 2 x 75753 and 255 x 6, encoded here: step 300 and an unclamped
    lut[255] of 256, which the kernel, like Pillow, clips; ten histogram workgroups per view"""
    ch = np.concatenate([np.full(1, 0), np.full(1000, 1), np.full(75753, 2), np.full(6, 255)]).astype(np.uint8)
    rng = np.random.default_rng(5)
    img = np.ascontiguousarray(np.stack([rng.permutation(ch).reshape(202, 380) for _ in range(3)], axis=-1))
    one = _Files([bytes(p) for p in _encode_gpu(enc, [(img, 0)])], [(380, 202)], [3])
    assert np.array_equal(one.planes[0][:3], img.transpose(2, 0, 1))  # (the reference decoder's bytes)
    assert TM.equalize_entries(TM.histograms(one.planes[0])[0])[255] == 256
    m = _Model(one)
    for layout, dtype, device in (("planar", "uint8", True), ("hwc", "float16", False)):
        kinds = PLANAR_KINDS if layout == "planar" else HWC_KINDS
        plan = [(3, [((0, 0, 380, 202), (380, 202), None, "bilinear", k == 1, kinds[k % len(kinds)]) for k in range(2)])]
        _run(enc, one, m, layout, [0], plan, dtype, device, None, None, None, [[EQUAL, EQUAL]])


# ---- 2. the guarantees: calls against each other ----
@pytest.mark.parametrize("dtype", ["uint8", "float16"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_records_without_an_op_are_the_warp_call(enc, files, layout, dtype):  # noqa: F811
    """GUARANTEES 1 and 2 on the warp test's batch (counts 1, 10, 1; both warp filters, blurs, point operations, direct views, mirrors,
    three and four channels): the buffer after the tone call with records without an op equals the buffer after the warp call, whole
    and bit for bit -- with matrices and with NULL colours, host and device files"""
    for device in (True, False):
        idx, plan, post, warp = _warp_plan(files, layout, VM.FILTERS[device], int(device))
        pngs = [files.pngs[i] for i in idx]
        dev = _device_files(pngs, shift=1) if device else None
        for color in (_matrices(plan, 70 + device), None):
            want = _warp_decode(enc, layout, pngs, plan, dtype, device, color, post, warp, dev=dev)
            assert not (want[1] == want[1][0]).all()  # (something was written)
            got = _decode(enc, layout, pngs, plan, dtype, device, color, post, warp, [[{}] * len(views) for _, views in plan], dev=dev)
            assert [(st, cf) for st, _, cf in got[0]] == [(st, cf) for st, _, cf in want[0]] == [(0, files.chans[i]) for i in idx]
            assert np.array_equal(got[1], want[1]), (device, color is None, int(np.count_nonzero(got[1] != want[1])))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_a_view_does_not_depend_on_the_files_other_views(enc, files, model, layout):  # noqa: F811
    """GUARANTEE 3: the fifteen views of the 600 x 130 file in the opposite order (other record numbers, other offsets in the scratch,
    other histograms), and three of them as the file's only view: the same elements (all against the model)"""
    idx, plan, color, post, warp, tone = _tone_plan(files, layout, "bicubic", 1)
    c, views = plan[1]
    _run(enc, files, model, layout, [idx[1]], [(c, views[::-1])], "float16", True, [color[1][::-1]], [post[1][::-1]], [warp[1][::-1]], [tone[1][::-1]])
    for k in (1, 3, 7):
        _run(enc, files, model, layout, [idx[1]], [(c, [views[k]])], "float16", True, [[color[1][k]]], [[post[1][k]]], [[warp[1][k]]], [[tone[1][k]]])


def test_a_tone_call_twice_gives_the_same(enc, files, model):  # noqa: F811
    """the histograms in the scratch are zeroed in front of every count: the same call twice into fresh buffers, the same buffers"""
    idx, plan, color, post, warp, tone = _tone_plan(files, "planar", "bilinear", 0)
    pngs = [files.pngs[i] for i in idx]
    dev = _device_files(pngs, shift=1)
    first = _decode(enc, "planar", pngs, plan, "uint8", True, color, post, warp, tone, dev=dev)
    again = _decode(enc, "planar", pngs, plan, "uint8", True, color, post, warp, tone, dev=dev)
    assert [st for st, _, _ in first[0]] == [st for st, _, _ in again[0]] == [0] * len(idx)
    assert np.array_equal(first[1], again[1]) and not (first[1] == first[1][0]).all()
    assert _difference("planar", again[1], "uint8", again[3], _sources(model, idx, plan, "uint8", color, post, warp, tone)) is None


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_a_damaged_file_leaves_the_others_views_unchanged(enc, files, model, layout, device):  # noqa: F811
    """a damaged file with tone records between good ones: its status is the plain views call's, nothing of its destinations is
    written, and every view of every other file is exact"""
    import torch
    kinds = PLANAR_KINDS if layout == "planar" else HWC_KINDS
    dtype = "float16" if device else "uint8"
    damaged = None
    for p in _damaged_files():
        w, h = _header_dims(p)
        if not (2 <= w <= 600 and 2 <= h <= 600):
            continue
        dviews = [((0, h - 2, w, 2), (max(w // 3, 2), 3), None, "bicubic", True, "odd"), ((0, 0, min(w, 5), 1), (3, 3), (1, 1, 2, 2), "bilinear", False, kinds[0])]
        nest = [[[v[k] for v in dviews]] for k in range(4)]
        planar = [[torch.full((3,) + _window(v[1], v[2])[:1:-1], SENTINEL, dtype=torch.uint8, device="cuda") for v in dviews]]
        (st, _, _), = enc.decode_batch_views([p], nest[0], planar, nest[1], nest[2], nest[3])
        torch.cuda.synchronize()
        # (a file that is refused before its resize is launched: the plain call leaves its destinations alone, so must this one)
        if st not in (0, UNDECIDED) and all(bool((t == SENTINEL).all()) for t in planar[0]):
            damaged = (p, dviews, st)
            break
    assert damaged is not None
    idx, plan, color, post, warp, tone = _tone_plan(files, layout, "bilinear", int(device))
    plan.insert(1, (3, damaged[1]))
    post.insert(1, [{}, {"solarize": 3}])
    warp.insert(1, [{"a": [1.0, 0.1, 0.0, 0.0, 1.0, 0.0], "filter": "bilinear", "fill": (1, 1, 1, 1)}, {}])
    tone.insert(1, [EQUAL, {"contrast": 1.3}])
    color.insert(1, _matrices([plan[1]], 11)[0])
    pngs = [files.pngs[idx[0]], damaged[0]] + [files.pngs[i] for i in idx[1:]]
    got, host, outs, regs = _decode(enc, layout, pngs, plan, dtype, device, color, post, warp, tone)
    assert [st for st, _, _ in got] == [0, damaged[2], 0, 0] and got[1][1] is None
    # (the damaged file's sources are None: its regions are expected to be all sentinel)
    diff = _difference(layout, host, dtype, regs, _sources(model, [idx[0], None] + idx[1:], plan, dtype, color, post, warp, tone, skip=(1,)))
    assert diff is None, diff


def test_a_descriptor_carries_its_records_and_decodes_again(enc, files, model):  # noqa: F811
    """make_decode_batch_views(..., tone=) once, decoded twice over overwritten outputs: the same both times; tone= next to a
    descriptor is refused"""
    import torch
    import fpng_amd
    idx, plan, color, post, warp, tone = _tone_plan(files, "planar", "bilinear", 0)
    dev = _device_files([files.pngs[i] for i in idx], shift=2)
    outs = [[torch.zeros((c,) + _window(full, window)[:1:-1], dtype=torch.float32, device="cuda") for _, full, window, *_ in views] for c, views in plan]
    nest = [[[v[k] for v in views] for _, views in plan] for k in range(5)]
    db = enc.make_decode_batch_views(dev, nest[0], outs, nest[1], nest[2], nest[3], mirror=nest[4], scale=CONSTS[0][0], bias=CONSTS[0][1], post=_post_records(post),
                                     warp=_warp_records(warp), tone=_tone_records(tone))
    want = _sources(model, idx, plan, "float32", None, post, warp, tone)
    for again in range(2):
        for ts in outs:
            for t in ts:
                t.fill_(1)
        assert enc.decode_device_views(db, results=False) is db
        torch.cuda.synchronize()
        assert list(db.statuses()) == [0] * len(idx)
        for k, t in enumerate(t for ts in outs for t in ts):
            assert np.array_equal(t.cpu().view(torch.uint8).numpy().view(np.uint32), want[k].transpose(2, 0, 1)), (again, k)
    with pytest.raises(ValueError):
        enc.decode_device_views(db, tone=fpng_amd.view_tone(equalize=True))
