"""GPU decoder of several resized views of each file THROUGH A PER-VIEW RESAMPLE RECORD (-m gpu;
fpng_amd_decode_batch(_device)_planar_views_resample and _hwc_views_resample: the alpha call, and for a launch that holds a view
with a RESAMPLE filter the resample instantiations of dec_resize_exact_kernel, dec_resize_hwc_kernel and dec_resize_color_kernel --
Pillow's NEAREST, BOX, HAMMING and LANCZOS next to bilinear and bicubic): the shapes of resample_model.VIEWS -- shrink in x with grow
in y, the evaluation window, the far corner, 1 x 1 windows at both ends, an upscale, the identity, 1 x 1 -> 5 x 5, and each filter's
exact scale limit, where the tiles sit on resize_max_taps, resize_tile_rows and resize_tile_lds -- in both layouts, uint8 and a float
dtype, mirrored and not; behind a colour matrix, in front of a blur, under COMPOSITE alpha; five filters in one file; a label map.

Expected values never come from the library: the bytes are the REFERENCE's decoder's, through resample_model.py (which
test_views_resample_cpu.py pins to Pillow) and the later stages' models.  The guarantee test alone compares two calls of the library
with each other.  Every call decodes into ONE sentinel-filled buffer that is compared WHOLE and bit for bit."""
import numpy as np
import pytest

from test_gpu_decode import _device_files
from test_gpu_decode_float import CONSTS
from test_gpu_decode_layouts import SENTINEL, _encode_gpu
from test_gpu_decode_planar import KINDS as PLANAR_KINDS, _Region as _PlanarRegion
from test_gpu_decode_resize import BITS, ELEM, _Files, enc  # noqa: F401  (enc: a fixture)
from test_gpu_decode_views_alpha import _Model, _alpha_records
from test_gpu_decode_views_color import LAYOUTS, _difference, _matrices
from test_gpu_decode_views_hwc import KINDS as HWC_KINDS, _Region as _HwcRegion
from test_gpu_decode_views_post import _records as _post_records
from test_gpu_resize_view import _window
import alpha_model as AM
import resample_model as SM

pytestmark = pytest.mark.gpu

NONE, TEAL = {}, {"op": "composite", "background": (12, 200, 177)}
NOISE, RGBA, ONE, LABELS = range(4)  # the files of the fixture, by index
LABEL_COLOURS = np.array([[0, 0, 0], [128, 0, 0], [0, 128, 0], [128, 128, 0], [0, 0, 128], [220, 20, 60]], dtype=np.uint8)  # (a palette of class colours)


def label_map(w, h):
    """(h, w, 3) uint8: blocks of 37 x 11 pixels of LABEL_COLOURS and a diagonal line one pixel wide"""
    y, x = np.mgrid[0:h, 0:w]
    k = (x // 37 + 2 * (y // 11)) % (len(LABEL_COLOURS) - 1)
    k[(x - 3 * y) % 97 == 0] = len(LABEL_COLOURS) - 1
    return LABEL_COLOURS[k]


@pytest.fixture(scope="module")
def rfiles(enc):  # noqa: F811
    """a 3-channel 600 x 130 noise file, alpha_model's 4-channel pattern at 600 x 130 (stored), a 1 x 1 file, the label map"""
    import fpng_amd
    items = [(fpng_amd.synth_image("noise", 600, 130, 3, seed=11), 0), (AM.pattern(600, 130, 3), 2), (np.array([[[200, 100, 50]]], dtype=np.uint8), 0), (label_map(600, 130), 0)]
    pngs = [bytes(p) for p in _encode_gpu(enc, items)]
    f = _Files(pngs, [(im.shape[1], im.shape[0]) for im, _ in items], [im.shape[2] for im, _ in items])
    for i, (im, _) in enumerate(items):  # (the reference decoder gives the images back)
        assert np.array_equal(f.planes[i][:im.shape[2]], im.transpose(2, 0, 1))
    return f


@pytest.fixture(scope="module")
def rmodel(rfiles):
    return _Model(rfiles)


def _names(f):
    """a plan's filter -> (filter=, resample=) of the call: a RESAMPLE filter overrides whichever filter the view has"""
    return (("bicubic" if f in ("box", "lanczos") else "bilinear"), f) if f in SM.NEW_FILTERS else (f, None)


def _decode(enc, layout, pngs, plan, dtype, device, alpha=None, color=None, post=None, resample=True, consts=CONSTS[0]):  # noqa: F811
    """plan: per file (c, [(crop, full, window, filter, mirror, kind)]), filter any of the six names; resample: True -- resample= from
    the plan's filters; "zero" -- records without a filter; None -- no resample= at all.  ONE call into ONE sentinel-filled buffer ->
    (results, the buffer afterwards, the tensors, the regions in the records' order)"""
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
            [[_names(v[3])[0] for v in views] for _, views in plan])
    kw.update(mirror=[[v[4] for v in views] for _, views in plan], order=[[r.order() for r in rs] for rs in per], bottom_up=[[r.kind == "bottom_up" for r in rs] for rs in per])
    if resample is True:
        kw["resample"] = [[_names(v[3])[1] for v in views] for _, views in plan]
    elif resample == "zero":
        kw["resample"] = [[None for _ in views] for _, views in plan]
    if alpha is not None:
        kw["alpha"] = _alpha_records(alpha)
    if post is not None:
        kw["post"] = _post_records(post)
    if color is not None:
        kw["color"] = color
    if device:
        call = enc.decode_device_views if layout == "planar" else enc.decode_device_views_hwc
        got = call(_device_files(pngs, shift=1), *args, **kw)
    else:
        call = enc.decode_batch_views if layout == "planar" else enc.decode_batch_views_hwc
        got = call(pngs, *args, **kw)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    return got, (host.view(BITS[e]) if layout == "planar" else host), outs, regs


def _sources(rmodel, idx, plan, dtype, alpha=None, color=None, post=None, consts=CONSTS[0]):
    """the (oh, ow, c) element bits of every view, in the records' order"""
    return [AM.view_elements(rmodel.view(idx[n], crop, full, window, f, NONE if alpha is None else alpha[n][k]), c, dtype, m, None if color is None else color[n][k], consts,
                             {} if post is None else post[n][k], {}, {}, {})
            for n, (c, views) in enumerate(plan) for k, (crop, full, window, f, m, _) in enumerate(views)]


def _run(enc, rfiles, rmodel, layout, idx, plan, dtype, device, alpha=None, color=None, post=None, consts=CONSTS[0]):  # noqa: F811
    got, host, outs, regs = _decode(enc, layout, [rfiles.pngs[i] for i in idx], plan, dtype, device, alpha, color, post, consts=consts)
    assert len(got) == len(idx)
    for n, (i, (st, views, cf)) in enumerate(zip(idx, got)):
        assert st == 0 and cf == rfiles.chans[i] and len(views) == len(outs[n]) and all(a is b for a, b in zip(views, outs[n])), (n, i, st, cf)
    diff = _difference(layout, host, dtype, regs, _sources(rmodel, idx, plan, dtype, alpha, color, post, consts))
    assert diff is None, (layout, dtype, device, diff)
    return host, regs


def _kinds(layout):
    return PLANAR_KINDS if layout == "planar" else HWC_KINDS


def _model_plan(layout, filter, flip):
    """every view of resample_model.VIEWS that `filter` has, of the 600 x 130 noise file and of the 1 x 1 file"""
    kinds = _kinds(layout)
    plan = []
    for dims in ((600, 130), (1, 1)):
        views = [v for v in SM.VIEWS[dims] if filter in v[3]]
        plan.append((3 + (flip ^ (dims == (1, 1))), [(crop, full, window, filter, flip ^ bool(k & 1), kinds[(k + flip) % len(kinds)]) for k, (crop, full, window, _) in enumerate(views)]))
    return [NOISE, ONE], plan


# ---- 1. every element against the model ----
@pytest.mark.parametrize("filter", SM.NEW_FILTERS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_the_views_of_the_model(enc, rfiles, rmodel, layout, filter):  # noqa: F811
    """resample_model.VIEWS under one filter, ONE call: uint8 from host files, float16 from device files with every mirror flag, the
    plane counts and the destination kinds flipped.  The views at the filter's exact limit -- 96 x 64 -> 3 x 2, or 9 x 6 under
    Lanczos -- have the most taps, rows and LDS that the filter's bounds allow"""
    for flip, dtype in ((False, "uint8"), (True, "float16")):
        idx, plan = _model_plan(layout, filter, flip)
        _run(enc, rfiles, rmodel, layout, idx, plan, dtype, flip, consts=CONSTS[flip])


@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_filter_in_one_file(enc, rfiles, rmodel, layout):  # noqa: F811
    """one file with a view per RESAMPLE filter, a bilinear view without a record's filter and a bicubic one: one decode of the union
    of their boxes, one launch, every view its own filter's"""
    kinds = _kinds(layout)
    filters = SM.NEW_FILTERS + ("bilinear", "bicubic")
    shapes = [((300, 40, 300, 90), (112, 112), None), ((0, 0, 256, 130), (256, 256), (16, 16, 224, 224)), ((100, 10, 450, 100), (150, 33), (85, 16, 65, 17))]
    plan = [(3, [(crop, full, window, f, bool(k & 1), kinds[k % len(kinds)]) for k, f in enumerate(filters) for crop, full, window in (shapes[k % 3],)])]
    _run(enc, rfiles, rmodel, layout, [NOISE], plan, "uint8", True)
    plan = [(4, [(shapes[0][0], shapes[0][1], None, f, False, kinds[0]) for f in filters])]  # (the same source box: the filters alone differ)
    _run(enc, rfiles, rmodel, layout, [RGBA], plan, "float32", False, consts=CONSTS[1])
    full = [rmodel.view(RGBA, shapes[0][0], shapes[0][1], None, f, NONE).tobytes() for f in filters]
    assert len(set(full)) == len(filters)  # (no two filters give the same image)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_behind_a_matrix_in_front_of_a_blur_and_under_a_composite(enc, rfiles, rmodel, layout):  # noqa: F811
    """the stages around the resize see a RESAMPLE filter's bytes as they see bilinear's: a colour matrix (the colour kernel), a blur
    of radius 1 (a post call: the resize writes the window into the scratch), COMPOSITE alpha on the RGBA file (the load of the
    horizontal pass) with a view without an op beside it, three and four planes"""
    kinds = _kinds(layout)
    shapes = [((0, 0, 600, 130), (224, 224), (150, 200, 74, 24)), ((5, 7, 9, 11), (65, 17), None), ((0, 0, 600, 130), (300, 65), (235, 48, 65, 17)), ((0, 0, 96, 64), (9, 6), None)]
    for c in (3, 4):
        plan = [(c, [(crop, full, window, f, bool((k + c) & 1), kinds[(k + c) % len(kinds)]) for k, (f, (crop, full, window)) in enumerate(zip(SM.NEW_FILTERS, shapes))])]
        alpha = [[TEAL, NONE, TEAL, TEAL]]
        color = _matrices(plan, 900 + c)
        _run(enc, rfiles, rmodel, layout, [RGBA], plan, "uint8", c == 3, alpha, color)
        _run(enc, rfiles, rmodel, layout, [NOISE], plan, "uint8", c == 4, None, color)
        post = [[{"blur": (1, 0.8)}, {}, {"blur": (1, 2.0)}, {}]]
        _run(enc, rfiles, rmodel, layout, [RGBA], plan, ("float16", "uint8")[c - 3], c == 4, alpha, None, post)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_a_label_map_keeps_its_colours(enc, rfiles, rmodel, layout):  # noqa: F811
    """the label map through NEAREST, shrunk, grown and mirrored: the views equal the model and hold the file's colours alone; the
    same views through bilinear hold others"""
    kinds = _kinds(layout)
    shapes = [((0, 0, 600, 130), (224, 224), None), ((30, 20, 500, 100), (256, 256), (16, 16, 224, 224)), ((100, 30, 57, 41), (171, 123), (50, 40, 65, 17))]
    plan = [(3, [(crop, full, window, "nearest", bool(k & 1), kinds[k % len(kinds)]) for k, (crop, full, window) in enumerate(shapes)])]
    _run(enc, rfiles, rmodel, layout, [LABELS], plan, "uint8", True)
    palette = {tuple(c) for c in LABEL_COLOURS.tolist()}
    for f, inside in (("nearest", True), ("bilinear", False)):
        got = [rmodel.view(LABELS, crop, full, window, f, NONE)[:3].reshape(3, -1).T for crop, full, window in shapes]
        assert all(({tuple(p) for p in np.unique(g, axis=0).tolist()} <= palette) == inside for g in got), f


# ---- 2. the guarantee: calls against each other ----
@pytest.mark.parametrize("layout", LAYOUTS)
def test_records_without_a_filter_are_the_alpha_call(enc, rfiles, layout):  # noqa: F811
    """with records whose filter is 0 the buffer after the resample call equals the buffer after the alpha call, whole and bit for
    bit: bilinear and bicubic views, a composite among them, host and device files"""
    kinds = _kinds(layout)
    shapes = [((0, 0, 600, 130), (224, 224), None), ((0, 0, 600, 130), (300, 65), (235, 48, 65, 17)), ((5, 7, 9, 11), (65, 17), None)]
    plan = [(c, [(crop, full, window, ("bilinear", "bicubic")[(k + c) % 2], bool(k & 1), kinds[(k + c) % len(kinds)]) for k, (crop, full, window) in enumerate(shapes)]) for c in (3, 4)]
    alpha = [[TEAL, NONE, TEAL], [NONE, TEAL, NONE]]
    for device in (False, True):
        pngs = [rfiles.pngs[RGBA], rfiles.pngs[NOISE]]
        want = _decode(enc, layout, pngs, plan, "uint8", device, alpha, resample=None)
        got = _decode(enc, layout, pngs, plan, "uint8", device, alpha, resample="zero")
        assert [(st, cf) for st, _, cf in got[0]] == [(st, cf) for st, _, cf in want[0]] == [(0, 4), (0, 3)]
        assert not (want[1] == want[1][0]).all() and np.array_equal(got[1], want[1]), (device, int(np.count_nonzero(got[1] != want[1])))
