"""GPU decoder of several resized views of each file THROUGH A PER-VIEW ENHANCE RECORD (-m gpu;
fpng_amd_decode_batch(_device)_planar_views_enhance and _hwc_views_enhance: the tone call, and for a call with an op the kMode == 3
instantiations of dec_view_post_kernel -- brightness composed into the tables in LDS, color blended behind the look-up of a
sample's three planes, sharpness filtered in LDS out of a tile loaded with a halo one wider than the blur's): the three operations on
windows of 1 x 1, 3 x 2 (no filter), 3 x 3 (one interior sample), one tile, a tile and a frame column and row more, and nine tiles;
planar and channels-last destinations, uint8 and the three float dtypes, three and four channels, mirrors, host and device files,
behind tone operations and warps of both filters, in front of blurs and point operations; enhance, tone-only, post-only and
direct views mixed in one file.

Expected values never come from the library: the bytes are the REFERENCE's decoder's, resized by resize_view_model.py, coloured by
color_model.py, warped by warp_model.py, toned by tone_model.py, enhanced by enhance_model.py and post-processed by post_model.py
(exact restatements; test_views_enhance_cpu.py holds enhance_model against the host twin and Pillow).  The guarantee tests alone
compare calls of the library with each other, as the guarantees say.  Every call decodes into ONE sentinel-filled buffer that is
compared WHOLE and bit for bit.

An enhance record here is enhance_model's dict: {"brightness": f}, {"color": f} or {"sharpness": f}, {} for a view without an op;
tone, warp and post records are tone_model's, warp_model's and post_model's dicts."""
import numpy as np
import pytest

from test_gpu_decode import UNDECIDED, _device_files
from test_gpu_decode_float import CONSTS
from test_gpu_decode_layouts import SENTINEL, _damaged_files, _header_dims
from test_gpu_decode_planar import KINDS as PLANAR_KINDS, _Region as _PlanarRegion
from test_gpu_decode_resize import BITS, DTYPES, ELEM, enc, files  # noqa: F401  (enc, files: fixtures)
from test_gpu_decode_views_color import LAYOUTS, _difference, _matrices
from test_gpu_decode_views_hwc import KINDS as HWC_KINDS, _Region as _HwcRegion
from test_gpu_decode_views_post import _records as _post_records
from test_gpu_decode_views_tone import AUTO, EQUAL, _decode as _tone_decode, _tone_plan, _tone_records
from test_gpu_decode_views_warp import W3, W64, W65, W130, _matrix, _warp_records
from test_gpu_resize_view import _window, model  # noqa: F401  (model: a fixture)
import enhance_model as EM
import resize_view_model as VM

pytestmark = pytest.mark.gpu

W33 = (50, 30, 3, 3)  # (exactly one interior sample)
OPS = ("brightness", "color", "sharpness")


def _enhance_records(enhance):
    import fpng_amd
    return [[fpng_amd.view_enhance(**p) for p in ps] for ps in enhance]


def _decode(enc, layout, pngs, plan, dtype, device, color, post, warp, tone, enhance, dev=None, consts=CONSTS[0]):  # noqa: F811
    """test_gpu_decode_views_tone's _decode with enhance= (per file a list of an enhance record per view; post, warp, tone None: no
    post=, warp=, tone= at all): ONE call into ONE sentinel-filled buffer -> (results, the buffer afterwards, the tensors, the regions
    in the records' order)"""
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
    kw["enhance"] = _enhance_records(enhance)
    if tone is not None:
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


def _sources(model, idx, plan, dtype, color, post, warp, tone, enhance, skip=(), consts=CONSTS[0]):  # noqa: F811
    """the (oh, ow, c) element bits of every view under its matrix (color None: the identity), warp (None: none), tone (None: none),
    enhance and post record (None: no flags), in the records' order (None for the views of the files in `skip`)"""
    return [None if n in skip else EM.view_elements(model.view(idx[n], crop, full, window, f), c, dtype, m, None if color is None else color[n][k], consts,
                                                    {} if post is None else post[n][k], {} if warp is None else warp[n][k], {} if tone is None else tone[n][k],
                                                    enhance[n][k])
            for n, (c, views) in enumerate(plan) for k, (crop, full, window, f, m, _) in enumerate(views)]


def _run(enc, files, model, layout, idx, plan, dtype, device, color, post, warp, tone, enhance, **kw):  # noqa: F811
    got, host, outs, regs = _decode(enc, layout, [files.pngs[i] for i in idx], plan, dtype, device, color, post, warp, tone, enhance, **kw)
    assert len(got) == len(idx)
    for n, (i, (st, views, cf)) in enumerate(zip(idx, got)):
        assert st == 0 and cf == files.chans[i] and len(views) == len(outs[n]) and all(a is b for a, b in zip(views, outs[n])), (n, i, st, cf)
    diff = _difference(layout, host, dtype, regs, _sources(model, idx, plan, dtype, color, post, warp, tone, enhance, consts=kw.get("consts", CONSTS[0])))
    assert diff is None, (layout, dtype, device, diff)


def _enhance_plan(files, layout, filter, k0):  # noqa: F811
    """counts 3, 37, 1: a 1 x 1 file under the three operations (the stage with a single sample), a 4-channel 600 x 130 file (k0 odd:
    the `noise` one) with thirty-seven views -- every operation alone on every window (W3: h < 3, sharpness is the identity; W33: one
    interior sample; W64: one tile; W65: a last tile of one frame column and row, whose neighbour's last interior column reads
    across the seam; W130: interior seams); behind a tone operation of each kind; behind a warp of either filter that leaves fill
    inside the window (fill samples are neighbours); in front of a blur of R = 1 and of R = 16, sharpness with R = 16 on W65 and
    R = 2 on W33 (R = min(w, h) - 1: the clamped outer ring); in front of solarize and posterize; a tone-only, a post-only and a
    direct view between them -- and a 3-channel 600 x 130 file at its own size (nine tile rows) sharpened behind a tone operation and
    in front of a blur, whose fourth plane, when it has one, skips the stage.  k0 flips every mirror flag and swaps three and four
    channels.  -> idx, plan, color, post, warp, tone, enhance"""
    flip = bool(k0 & 1)
    kinds = PLANAR_KINDS if layout == "planar" else HWC_KINDS
    i600, whole, full = (5 if flip else 4), (0, 0, 600, 130), (300, 65)
    assert files.dims[i600] == (600, 130) and files.chans[i600] == 4 and files.dims[14 + flip] == (1, 1) and files.dims[2] == (600, 130) and files.chans[2] == 3
    near, lin = "nearest", "bilinear"
    big = (0, 0, 600, 130)  # (a window of the file at its own size: the full one)
    factors = (1.8, 0.4, 2.5, 0.0, 3.0)
    # (window, mirror, post, warp, tone, enhance)
    views = [(win, bool((k + n) & 1), {}, {}, {}, {op: factors[(k + n) % 5]}) for n, win in enumerate((W3, W33, W64, W65, W130)) for k, op in enumerate(OPS)]
    views += [(W130, False, {}, {}, AUTO, {"sharpness": 2.0}),
              (W65, True, {}, {}, EQUAL, {"color": 1.7}),
              (W64, False, {}, {}, {"contrast": 1.6}, {"brightness": 0.6}),
              (W33, True, {}, {}, EQUAL, {"sharpness": 0.0}),
              (W130, False, {}, {"a": _matrix(W130, angle=30.0), "filter": near, "fill": (10, 20, 30, 40)}, {}, {"sharpness": 2.2}),
              (W65, True, {}, {"a": [1.0, 0.37, -2.5, 0.0, 1.0, 0.0], "filter": lin, "fill": (255, 0, 128, 7)}, {}, {"color": 0.3}),
              (W64, False, {}, {"a": _matrix(W64, angle=-10.0), "filter": lin, "fill": (9, 99, 199, 0)}, {"contrast": 1.5}, {"brightness": 1.4}),
              (W130, True, {"blur": (16, 5.0)}, {}, {}, {"sharpness": 1.9}),
              (W130, False, {"blur": (1, 0.5)}, {}, {}, {"color": 2.0}),
              (W65, False, {"blur": (16, 4.0)}, {}, {}, {"sharpness": 2.5}),
              (W33, False, {"blur": (2, 1.0)}, {}, {}, {"sharpness": 3.0}),
              (W64, True, {"blur": (1, 2.0)}, {"a": _matrix(W64, angle=45.0), "filter": near, "fill": (1, 2, 3, 4)}, AUTO, {"sharpness": 0.5}),
              (W130, False, {"blur": (16, 3.0), "solarize": 100}, {}, {"contrast": 0.4}, {"brightness": 1.3}),
              (W3, True, {"blur": (1, 2.0)}, {}, {}, {"sharpness": 2.0}),
              (W65, True, {"solarize": 100}, {}, {}, {"sharpness": 1.5}),
              (W64, False, {"posterize": 3}, {}, {}, {"color": 1.5}),
              (W65, False, {"solarize": 128, "posterize": 5}, {"a": _matrix(W65, angle=10.0, translate=(2.5, -1.25)), "filter": lin, "fill": (200, 100, 50, 25)}, EQUAL,
               {"sharpness": 1.8}),
              (W130, False, {"blur": (11, 1.3), "posterize": 3}, {}, {}, {}),
              (W65, True, {}, {}, AUTO, {}),
              (W65, False, {"blur": (16, 4.0)}, {}, {}, {}),
              (W65, True, {}, {}, {}, {}),
              (W130, True, {"blur": (3, 1.0)}, {}, {}, {"color": 0.0})]
    idx = [14 + flip, i600, 2]
    plan = [(3 + flip, [((0, 0, 1, 1), (1, 1), None, filter, flip ^ bool(k & 1), kinds[(k0 + k) % len(kinds)]) for k in range(3)]),
            (4 - flip, [(whole, full, w, filter, m ^ flip, kinds[(k0 + k) % len(kinds)]) for k, (w, m, *_) in enumerate(views)]),
            (3 + flip, [(whole, (600, 130), big, filter, not flip, kinds[(k0 + 2) % len(kinds)])])]
    post = [[{}, {"solarize": 100}, {}], [v[2] for v in views], [{"blur": (16, 2.0)}]]
    warp = [[{}] * 3, [v[3] for v in views], [{}]]
    tone = [[{}, {"contrast": 3.0}, {}], [v[4] for v in views], [(AUTO, EQUAL)[k0 % 2]]]
    enhance = [[{"brightness": 1.7}, {"color": 0.3}, {"sharpness": 2.0}], [v[5] for v in views], [{"sharpness": 1.6}]]
    color = _matrices(plan, 400 + k0)
    assert [len(v) for _, v in plan] == [3, 37, 1]
    return idx, plan, color, post, warp, tone, enhance


# ---- 1. every element against the model ----
@pytest.mark.parametrize("dtype", ["uint8", "float32"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_window_operation_tone_warp_and_post_mixed_with_views_without_enhance(enc, files, model, layout, dtype):  # noqa: F811
    """the batch of _enhance_plan plain and flipped: uint8 and float32 in both layouts, bilinear and bicubic resizes, host and device
    files, dealt so that each value of each meets both values of the others"""
    d = (dtype != "uint8") + LAYOUTS.index(layout)
    for k0 in (0, 1):
        idx, plan, color, post, warp, tone, enhance = _enhance_plan(files, layout, VM.FILTERS[(k0 + d) % 2], k0)
        if k0 == 0:  # (the plan does what its text says: fill inside the warped windows)
            assert not EM.WM.apply_plane(warp[1][19], np.ones((33, 130), np.uint8), False, 0).all() and not EM.WM.apply_plane(warp[1][20], np.ones((17, 65), np.uint8), False, 0).all()
        _run(enc, files, model, layout, idx, plan, dtype, bool((k0 + d + d // 2) & 1), color, post, warp, tone, enhance, consts=CONSTS[k0])


@pytest.mark.parametrize("dtype", [t for t in DTYPES if t not in ("uint8", "float32")])
def test_the_other_dtypes_on_one_shape(enc, files, model, dtype):  # noqa: F811
    """the other two float dtypes in both layouts on the 65 x 17 window: the three operations, mirrored and not, with and without
    posts, warps and tones (NULL posts, warps, tones and colours: the call's own records without flags)"""
    for layout in LAYOUTS:
        kinds = PLANAR_KINDS if layout == "planar" else HWC_KINDS
        whole, full = (0, 0, 600, 130), (300, 65)
        plan = [(4, [(whole, full, W65, "bilinear", bool(k & 1), kinds[k % len(kinds)]) for k in range(3)]), (4, [(whole, full, W65, "bicubic", True, kinds[-1])])]
        enhance = [[{"sharpness": 1.75}, {"color": 1.25}, {"brightness": 0.75}], [{"sharpness": 0.25}]]
        tone = [[AUTO, {}, EQUAL], [{"contrast": 0.75}]]
        warp = [[{"a": _matrix(W65, angle=-15.0, shear=(8.0, 0.0)), "filter": "bilinear", "fill": (1, 128, 255, 64)}, {}, {}],
                [{"a": [1.0, 0.0, 3.0, 0.0, 1.0, -2.0], "filter": "nearest", "fill": (0, 255, 0, 255)}]]
        post = [[{"blur": (2, 1.0)}, {"posterize": 4}, {}], [{"solarize": 77}]]
        for with_others in (True, False):
            _run(enc, files, model, layout, [4, 2], plan, dtype, not with_others, _matrices(plan, 90) if with_others else None, post if with_others else None,
                 warp if with_others else None, tone if with_others else None, enhance)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_factors_on_the_noise_file_clip_at_both_ends(enc, files, model, layout):  # noqa: F811
    """the three operations at the factors 0, 0.5, 1 and 2.5 on the nine-tile window of the `noise` file, and sharpness at 2.5 in front
    of a blur: at 2.5 color and sharpness clip at 0 and at 255"""
    kinds = PLANAR_KINDS if layout == "planar" else HWC_KINDS
    assert files.dims[5] == (600, 130) and files.chans[5] == 4
    enhance = [[{op: f} for op in OPS for f in (0.0, 0.5, 1.0, 2.5)] + [{"sharpness": 2.5}]]
    post = [[{}] * 12 + [{"blur": (1, 0.8)}]]
    plan = [(4, [((0, 0, 600, 130), (300, 65), W130, "bilinear", bool(k & 1), kinds[k % len(kinds)]) for k in range(13)])]
    want = _sources(model, [5], plan, "uint8", None, post, None, None, enhance)
    for k in (7, 11):
        assert (want[k][..., :3] == 0).any() and (want[k][..., :3] == 255).any(), k
    _run(enc, files, model, layout, [5], plan, "uint8", layout == "planar", None, post, None, None, enhance)


# ---- 2. the guarantees: calls against each other ----
@pytest.mark.parametrize("dtype", ["uint8", "float16"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_records_without_an_op_and_factors_of_one_are_the_tone_call(enc, files, layout, dtype):  # noqa: F811
    """GUARANTEES 1 to 3 on the tone test's batch (counts 3, 15, 1; all three tone operations, both warp filters, blurs, point
    operations, direct views, mirrors, three and four channels): the buffer after the enhance call with records without an op, and
    with each operation at factor 1 on every view, equals the buffer after the tone call, whole and bit for bit -- with matrices and
    with NULL colours, host and device files.  A view with an op is a post view: its float elements are the conversion of its BYTES,
    where a view without any record is converted from the matrix's unrounded result.  So the tone call that the factors of 1 are
    held against gives every view that has no record of its own a posterize to 8 bits -- the identity, and a post view"""
    for device in (True, False):
        idx, plan, color, post, warp, tone = _tone_plan(files, layout, VM.FILTERS[device], int(device))
        pngs = [files.pngs[i] for i in idx]
        dev = _device_files(pngs, shift=1) if device else None
        as_post = [[p if p or w or t else {"posterize": 8} for p, w, t in zip(ps, ws, ts)] for ps, ws, ts in zip(post, warp, tone)]
        assert as_post != post  # (the batch has direct views)
        for colors in (color, None):
            for posts, recs in ((post, [{}]), (as_post, [{op: 1.0} for op in OPS])):
                want = _tone_decode(enc, layout, pngs, plan, dtype, device, colors, posts, warp, tone, dev=dev)
                assert not (want[1] == want[1][0]).all()  # (something was written)
                for rec in recs:
                    got = _decode(enc, layout, pngs, plan, dtype, device, colors, posts, warp, tone, [[rec] * len(views) for _, views in plan], dev=dev)
                    assert [(st, cf) for st, _, cf in got[0]] == [(st, cf) for st, _, cf in want[0]] == [(0, files.chans[i]) for i in idx]
                    assert np.array_equal(got[1], want[1]), (device, colors is None, rec, int(np.count_nonzero(got[1] != want[1])))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_a_view_does_not_depend_on_the_files_other_views(enc, files, model, layout):  # noqa: F811
    """GUARANTEE 4: the views of the 600 x 130 file in the opposite order (other record numbers, other offsets in the scratch), and
    four of them as the file's only view: the same elements (all against the model)"""
    idx, plan, color, post, warp, tone, enhance = _enhance_plan(files, layout, "bicubic", 1)
    c, views = plan[1]
    _run(enc, files, model, layout, [idx[1]], [(c, views[::-1])], "float16", True, [color[1][::-1]], [post[1][::-1]], [warp[1][::-1]], [tone[1][::-1]], [enhance[1][::-1]])
    for k in (5, 19, 24, 25):
        _run(enc, files, model, layout, [idx[1]], [(c, [views[k]])], "float16", True, [[color[1][k]]], [[post[1][k]]], [[warp[1][k]]], [[tone[1][k]]], [[enhance[1][k]]])


def test_an_enhance_call_twice_gives_the_same(enc, files, model):  # noqa: F811
    idx, plan, color, post, warp, tone, enhance = _enhance_plan(files, "planar", "bilinear", 0)
    pngs = [files.pngs[i] for i in idx]
    dev = _device_files(pngs, shift=1)
    first = _decode(enc, "planar", pngs, plan, "uint8", True, color, post, warp, tone, enhance, dev=dev)
    again = _decode(enc, "planar", pngs, plan, "uint8", True, color, post, warp, tone, enhance, dev=dev)
    assert [st for st, _, _ in first[0]] == [st for st, _, _ in again[0]] == [0] * len(idx)
    assert np.array_equal(first[1], again[1]) and not (first[1] == first[1][0]).all()


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_a_damaged_file_leaves_the_others_views_unchanged(enc, files, model, layout, device):  # noqa: F811
    """a damaged file with enhance records between good ones: its status is the plain views call's, nothing of its destinations is
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
    idx, plan, color, post, warp, tone, enhance = _enhance_plan(files, layout, "bilinear", int(device))
    plan.insert(1, (3, damaged[1]))
    post.insert(1, [{}, {"solarize": 3}])
    warp.insert(1, [{"a": [1.0, 0.1, 0.0, 0.0, 1.0, 0.0], "filter": "bilinear", "fill": (1, 1, 1, 1)}, {}])
    tone.insert(1, [EQUAL, {}])
    enhance.insert(1, [{"sharpness": 1.3}, {"color": 0.5}])
    color.insert(1, _matrices([plan[1]], 11)[0])
    pngs = [files.pngs[idx[0]], damaged[0]] + [files.pngs[i] for i in idx[1:]]
    got, host, outs, regs = _decode(enc, layout, pngs, plan, dtype, device, color, post, warp, tone, enhance)
    assert [st for st, _, _ in got] == [0, damaged[2], 0, 0] and got[1][1] is None
    # (the damaged file's sources are None: its regions are expected to be all sentinel)
    diff = _difference(layout, host, dtype, regs, _sources(model, [idx[0], None] + idx[1:], plan, dtype, color, post, warp, tone, enhance, skip=(1,)))
    assert diff is None, diff


def test_a_descriptor_carries_its_records_and_decodes_again(enc, files, model):  # noqa: F811
    """make_decode_batch_views(..., enhance=) once, decoded twice over overwritten outputs: the same both times; enhance= next to a
    descriptor is refused"""
    import torch
    import fpng_amd
    idx, plan, color, post, warp, tone, enhance = _enhance_plan(files, "planar", "bilinear", 0)
    dev = _device_files([files.pngs[i] for i in idx], shift=2)
    outs = [[torch.zeros((c,) + _window(full, window)[:1:-1], dtype=torch.float32, device="cuda") for _, full, window, *_ in views] for c, views in plan]
    nest = [[[v[k] for v in views] for _, views in plan] for k in range(5)]
    db = enc.make_decode_batch_views(dev, nest[0], outs, nest[1], nest[2], nest[3], mirror=nest[4], scale=CONSTS[0][0], bias=CONSTS[0][1], post=_post_records(post),
                                     warp=_warp_records(warp), tone=_tone_records(tone), enhance=_enhance_records(enhance))
    want = _sources(model, idx, plan, "float32", None, post, warp, tone, enhance)
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
        enc.decode_device_views(db, enhance=fpng_amd.view_enhance(sharpness=2.0))
