"""GPU decoder of several resized views of each file THROUGH A PER-VIEW ALPHA RECORD (-m gpu;
fpng_amd_decode_batch(_device)_planar_views_alpha and _hwc_views_alpha: the enhance call, and for a launch with an op the alpha
instantiations of dec_resize_exact_kernel, dec_resize_hwc_kernel and dec_resize_color_kernel -- the composite or the premultiply in
the load of the horizontal pass, the division in the store of the vertical pass; a planar call with a PREMULTIPLIED view runs the
colour kernel under identity matrices, one with composites alone the per-plane kernel): windows of 1 x 1, one tile, a tile and a
column and row more, and seams, both filters, upscaling and downscaling, mirrors, uint8 and the three float dtypes, planar and channels-last destinations of three and
four planes in every pitch kind, host and device files, compressed and stored files; views of different ops and backgrounds in
one file; the bilinear LDS limit; behind a colour matrix, in front of a warp with fill and of a blur.

Expected values never come from the library: the bytes are the REFERENCE's decoder's, through alpha_model.py (which
test_views_alpha_cpu.py pins to Pillow) and the later stages' models.  The guarantee tests alone compare calls of the library with
each other, as the guarantees say.  Every call decodes into ONE sentinel-filled buffer that is compared WHOLE and bit for bit.

An alpha record here is alpha_model's dict: {}, {"op": "composite", "background": (r, g, b)} or {"op": "premultiplied"}."""
import numpy as np
import pytest

from test_gpu_decode import UNDECIDED, _device_files
from test_gpu_decode_float import CONSTS
from test_gpu_decode_layouts import SENTINEL, _damaged_files, _encode_gpu, _header_dims
from test_gpu_decode_planar import KINDS as PLANAR_KINDS, _Region as _PlanarRegion
from test_gpu_decode_resize import BITS, DTYPES, ELEM, _Files, enc  # noqa: F401  (enc: a fixture)
from test_gpu_decode_views_color import LAYOUTS, _difference, _matrices
from test_gpu_decode_views_enhance import _decode as _enhance_decode
from test_gpu_decode_views_hwc import KINDS as HWC_KINDS, _Region as _HwcRegion
from test_gpu_decode_views_post import _records as _post_records
from test_gpu_decode_views_warp import _matrix, _warp_records
from test_gpu_resize_view import _window
import alpha_model as AM
import resize_view_model as VM

pytestmark = pytest.mark.gpu

NONE, PRE = {}, {"op": "premultiplied"}
WHITE, BLACK = {"op": "composite", "background": (255, 255, 255)}, {"op": "composite", "background": (0, 0, 0)}
TEAL, ROSE = {"op": "composite", "background": (12, 200, 177)}, {"op": "composite", "background": (250, 3, 99)}
# the files of the fixture, by index
P90, P90S, P33, P33S, RGB90, ONE0, ONE128, NOISE = range(8)
WHOLE90, WHOLE33, WHOLE600 = (0, 0, 90, 40), (0, 0, 33, 9), (0, 0, 600, 130)
UP90, DOWN90 = (200, 90), (70, 30)  # full sizes of the 90 x 40 files
# windows: 1 x 1, one tile, a tile and a column and a row more, seams in both axes
W1, W64, W65, W130 = (199, 89, 1, 1), (3, 5, 64, 16), (100, 50, 65, 17), (60, 40, 130, 35)
D1, D64, D65 = (0, 29, 1, 1), (3, 7, 64, 16), (0, 3, 65, 17)


def _alpha_records(alpha):
    import fpng_amd
    return [[fpng_amd.view_alpha(**p) for p in ps] for ps in alpha]


@pytest.fixture(scope="module")
def afiles(enc):  # noqa: F811
    """the pattern of alpha_model.pattern as 4-channel 90 x 40 and 33 x 9 files, compressed and stored; a 3-channel 90 x 40 file;
    4-channel 1 x 1 files with alpha 0 and 128; a 4-channel 600 x 130 noise file.  Their planes: the reference decoder's"""
    import fpng_amd
    one = np.array([[[200, 100, 50, 0]]], dtype=np.uint8)
    half = np.array([[[200, 100, 50, 128]]], dtype=np.uint8)
    items = [(AM.pattern(90, 40, 1), 0), (AM.pattern(90, 40, 1), 2), (AM.pattern(33, 9), 0), (AM.pattern(33, 9), 2), (np.ascontiguousarray(AM.pattern(90, 40, 2)[..., :3]), 0),
             (one, 0), (half, 0), (fpng_amd.synth_image("noise", 600, 130, 4, seed=5), 2)]
    pngs = [bytes(p) for p in _encode_gpu(enc, items)]
    f = _Files(pngs, [(im.shape[1], im.shape[0]) for im, _ in items], [im.shape[2] for im, _ in items])
    for i, (im, _) in enumerate(items):  # (the reference decoder gives the images back)
        assert np.array_equal(f.planes[i][:im.shape[2]], im.transpose(2, 0, 1)) and (im.shape[2] == 4 or (f.planes[i][3] == 255).all())
    return f


def _check_conditions(afiles):
    """the conditions on the images (test_views_alpha_cpu.py holds them on the pattern; here on the reference decoder's planes)"""
    for i, full in ((P33, (70, 20)), (P33S, (70, 20)), (P90, UP90), (P90S, UP90)):
        got = AM.conditions(afiles.planes[i], full, "bicubic")
        assert all(got[k] >= 1 for k in ("clip", "zero_alpha_colour", "alpha_0", "alpha_255", "alpha_between")), (i, got)


class _Model:
    """R of (file, crop, full, filter, alpha): P' resized whole once each from the reference decoder's four planes; a view is U of a slice"""

    def __init__(self, files):
        self.files, self._full = files, {}

    def view(self, i, crop, full, window, filter, alpha):
        key = (i, crop, full, filter, alpha.get("op"), tuple(alpha.get("background", ())))
        if key not in self._full:
            x, y, w, h = crop
            r = AM.resized(alpha, self.files.planes[i][:, y:y + h, x:x + w], full, filter)
            r.setflags(write=False)
            self._full[key] = r
        x, y, w, h = _window(full, window)
        return AM.result(alpha, self._full[key][:, y:y + h, x:x + w])


@pytest.fixture(scope="module")
def amodel(afiles):
    return _Model(afiles)


def _decode(enc, layout, pngs, plan, dtype, device, alpha, color=None, post=None, warp=None, enhance=None, dev=None, consts=CONSTS[0]):  # noqa: F811
    """plan: per file (c, [(crop, full, window, filter, mirror, kind)]); alpha: per file a list of an alpha record per view (None: no
    alpha= at all); color, post, warp, enhance: None, or the same nesting.  ONE call into ONE sentinel-filled buffer -> (results, the
    buffer afterwards, the tensors, the regions in the records' order)"""
    import torch
    import fpng_amd
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
    if alpha is not None:
        kw["alpha"] = _alpha_records(alpha)
    if enhance is not None:
        kw["enhance"] = [[fpng_amd.view_enhance(**p) for p in ps] for ps in enhance]
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


def _sources(amodel, idx, plan, dtype, alpha, color=None, post=None, warp=None, skip=(), consts=CONSTS[0]):
    """the (oh, ow, c) element bits of every view, in the records' order (None for the views of the files in `skip`)"""
    return [None if n in skip else AM.view_elements(amodel.view(idx[n], crop, full, window, f, alpha[n][k]), c, dtype, m, None if color is None else color[n][k], consts,
                                                    {} if post is None else post[n][k], {} if warp is None else warp[n][k], {}, {})
            for n, (c, views) in enumerate(plan) for k, (crop, full, window, f, m, _) in enumerate(views)]


def _run(enc, afiles, amodel, layout, idx, plan, dtype, device, alpha, color=None, post=None, warp=None, **kw):  # noqa: F811
    got, host, outs, regs = _decode(enc, layout, [afiles.pngs[i] for i in idx], plan, dtype, device, alpha, color, post, warp, **kw)
    assert len(got) == len(idx)
    for n, (i, (st, views, cf)) in enumerate(zip(idx, got)):
        assert st == 0 and cf == afiles.chans[i] and len(views) == len(outs[n]) and all(a is b for a, b in zip(views, outs[n])), (n, i, st, cf)
    diff = _difference(layout, host, dtype, regs, _sources(amodel, idx, plan, dtype, alpha, color, post, warp, consts=kw.get("consts", CONSTS[0])))
    assert diff is None, (layout, dtype, device, diff)


def _alpha_plan(layout, k0):
    """The batch: the 90 x 40 pattern, compressed and stored, under every op on every window -- upscaled (both filters: under bicubic
    U's clip is live and R'_3 == 0 meets colour) and downscaled -- with views of four different backgrounds, a premultiplied view
    and views without an op between them in ONE file; the 33 x 9 pattern to 70 x 20, whole; the 3-channel file under every op; the
    1 x 1 files with alpha 0 and 128 (premultiplied: U copies, and divides by 128).  k0 flips every mirror flag, swaps the
    filters and three and four planes.  -> idx, plan, alpha"""
    flip = bool(k0 & 1)
    kinds = PLANAR_KINDS if layout == "planar" else HWC_KINDS
    fs = VM.FILTERS[::-1] if flip else VM.FILTERS
    ops = (WHITE, PRE, NONE, TEAL, PRE, ROSE, BLACK, NONE)
    # (full, window, op) of a 90 x 40 file: every window under a composite and under the premultiplied resize, ops interleaved
    views = [(UP90, w, ops[(n + k) % len(ops)]) for n, w in enumerate((W1, W64, W65, W130)) for k in (0, 1, 2)]
    views += [(DOWN90, w, ops[(n + k + 1) % len(ops)]) for n, w in enumerate((D1, D64, D65)) for k in (0, 1)]
    views += [(UP90, W130, PRE), (UP90, W65, TEAL), (DOWN90, None, PRE)]

    def file90(c, shift):
        return (c, [(WHOLE90, full, w, fs[(k + shift) % 2], flip ^ bool(k & 1), kinds[(k0 + k + shift) % len(kinds)]) for k, (full, w, _) in enumerate(views)])

    small = [(WHOLE33, (70, 20), None, fs[k % 2], flip ^ bool(k & 1), kinds[(k0 + k) % len(kinds)]) for k in range(4)]
    rgb = [(WHOLE90, UP90, W65, fs[k % 2], bool(k & 1), kinds[(k0 + 2 * k) % len(kinds)]) for k in range(3)]
    ones = [((0, 0, 1, 1), (5, 5), (1, 1, 3, 3), fs[k % 2], False, kinds[(k0 + k) % len(kinds)]) for k in range(3)]
    idx = [P90, P33, RGB90, ONE0, P90S, P33S, ONE128]
    plan = [file90(3 + flip, 0), (4 - flip, small), (3 + flip, rgb), (4 - flip, ones), file90(4 - flip, 1), (3 + flip, small[::-1]), (3 + flip, ones)]
    a90 = [v[2] for v in views]
    alpha = [a90, [PRE, PRE, WHITE, NONE], [WHITE, PRE, NONE], [PRE, TEAL, NONE], a90, [NONE, WHITE, PRE, PRE], [PRE, ROSE, NONE]]
    assert [len(v) for _, v in plan] == [len(a) for a in alpha]
    # (one file: composites over at least three backgrounds, a premultiplied view and a view without an op)
    assert len({tuple(a["background"]) for a in a90 if a.get("op") == "composite"}) >= 3 and PRE in a90 and NONE in a90
    return idx, plan, alpha


# ---- 1. every element against the model ----
@pytest.mark.parametrize("dtype", ["uint8", "float32"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_window_op_and_background_mixed_in_one_file(enc, afiles, amodel, layout, dtype):  # noqa: F811
    """the batch of _alpha_plan plain and flipped: uint8 and float32 in both layouts, host and device files"""
    _check_conditions(afiles)
    d = (dtype != "uint8") + LAYOUTS.index(layout)
    for k0 in (0, 1):
        idx, plan, alpha = _alpha_plan(layout, k0)
        _run(enc, afiles, amodel, layout, idx, plan, dtype, bool((k0 + d) & 1), alpha, consts=CONSTS[k0])
        if layout == "planar":  # (composites and views without an op alone: every window through the per-plane kernel's alpha instantiation)
            only = [[BLACK if a == PRE else a for a in row] for row in alpha]
            _run(enc, afiles, amodel, layout, idx, plan, dtype, not (k0 + d) & 1, only, consts=CONSTS[k0])


@pytest.mark.parametrize("dtype", [t for t in DTYPES if t not in ("uint8", "float32")])
def test_the_other_dtypes_on_one_shape(enc, afiles, amodel, dtype):  # noqa: F811
    """the other two float dtypes in both layouts on the 65 x 17 window, upscaled by both filters: every op, mirrored and not"""
    _check_conditions(afiles)
    for layout in LAYOUTS:
        kinds = PLANAR_KINDS if layout == "planar" else HWC_KINDS
        plan = [(c, [(WHOLE90, UP90, W65, VM.FILTERS[(k + c) % 2], bool(k & 1), kinds[(k + c) % len(kinds)]) for k in range(4)]) for c in (3, 4)]
        alpha = [[PRE, TEAL, NONE, PRE], [WHITE, PRE, PRE, NONE]]
        _run(enc, afiles, amodel, layout, [P90, P90S], plan, dtype, layout == "hwc", alpha)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_channels_last_kinds_and_plane_orders(enc, afiles, amodel, layout):  # noqa: F811
    """every destination kind of the layout -- for channels-last ones the reversed order and pixel_elems = 4 under three planes, whose
    fourth element stays the caller's -- under the premultiplied resize and a composite, three and four planes"""
    kinds = PLANAR_KINDS if layout == "planar" else HWC_KINDS
    plan = [(c, [(WHOLE33, (70, 20), (2, 1, 66, 18), "bicubic", bool(k & 1), kind) for k, kind in enumerate(kinds) for _ in (0, 1)]) for c in (3, 4)]
    alpha = [[(PRE, ROSE)[n] for _ in kinds for n in (0, 1)]] * 2
    _run(enc, afiles, amodel, layout, [P33, P33S], plan, "uint8", False, alpha)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_the_bilinear_lds_limit(enc, afiles, amodel, layout):  # noqa: F811
    """600 x 130 -> 19 x 5 under the bilinear filter: 65 taps in x, a tile of 55 KB of LDS -- the premultiplied view (four planes
    through the one T, whatever the destination has), a composite and a view without an op in one call, and composites alone (the
    per-plane kernel), three and four planes"""
    assert afiles.dims[NOISE] == (600, 130) and afiles.chans[NOISE] == 4
    kinds = PLANAR_KINDS if layout == "planar" else HWC_KINDS
    for c in (3, 4):
        plan = [(c, [(WHOLE600, (19, 5), None, "bilinear", bool(k & 1), kinds[k % len(kinds)]) for k in range(3)])]
        _run(enc, afiles, amodel, layout, [NOISE], plan, "uint8", c == 4, [[PRE, TEAL, NONE]])
        _run(enc, afiles, amodel, layout, [NOISE], plan, "uint8", c == 3, [[ROSE, TEAL, NONE]])


@pytest.mark.parametrize("layout", LAYOUTS)
def test_behind_a_matrix_in_front_of_a_warp_and_a_blur(enc, afiles, amodel, layout):  # noqa: F811
    """the later stages see R: a colour matrix alone (the colour call's launch); and in a post call a nearest warp with fill, a blur
    of R = 1, both, and direct views, over composited and premultiplied views, bytes and floats"""
    kinds = PLANAR_KINDS if layout == "planar" else HWC_KINDS
    for c in (3, 4):
        plan = [(c, [(WHOLE90, UP90, w, VM.FILTERS[k % 2], bool(k & 1), kinds[(k + c) % len(kinds)]) for k, w in enumerate((W64, W65, W130, W65, W64, W130))])]
        alpha = [[PRE, WHITE, PRE, NONE, TEAL, PRE]]
        color = _matrices(plan, 700 + c)
        _run(enc, afiles, amodel, layout, [P90], plan, "uint8", False, alpha, color)
        warp = [[{"a": _matrix(W64, angle=30.0), "filter": "nearest", "fill": (10, 20, 30, 40)}, {}, {}, {}, {}, {"a": _matrix(W130, angle=-20.0), "filter": "nearest", "fill": (255, 0, 7, 9)}]]
        post = [[{}, {"blur": (1, 0.8)}, {}, {"blur": (1, 2.0)}, {}, {"blur": (1, 0.5)}]]
        _run(enc, afiles, amodel, layout, [P90S], plan, ("float16", "uint8")[c - 3], True, alpha, color if c == 3 else None, post, warp)


# ---- 2. the guarantees: calls against each other ----
@pytest.mark.parametrize("layout", LAYOUTS)
def test_records_without_an_op_are_the_enhance_call(enc, afiles, layout):  # noqa: F811
    """GUARANTEE 1: with records without an op, the buffer after the alpha call equals the buffer after the enhance call, whole and
    bit for bit -- with enhance ops (a post call) and with none (the plain call's launch), host and device files"""
    for device in (False, True):
        idx, plan, _ = _alpha_plan(layout, int(device))
        pngs = [afiles.pngs[i] for i in idx]
        dev = _device_files(pngs, shift=1) if device else None
        none = [[NONE] * len(views) for _, views in plan]
        for enhance in ([[{} for _ in views] for _, views in plan], [[({"brightness": 1.5}, {}, {"sharpness": 2.0})[k % 3] for k, _ in enumerate(views)] for _, views in plan]):
            want = _enhance_decode(enc, layout, pngs, plan, "uint8", device, None, None, None, None, enhance, dev=dev)
            got = _decode(enc, layout, pngs, plan, "uint8", device, none, enhance=enhance, dev=dev)
            assert [(st, cf) for st, _, cf in got[0]] == [(st, cf) for st, _, cf in want[0]] == [(0, afiles.chans[i]) for i in idx]
            assert not (want[1] == want[1][0]).all() and np.array_equal(got[1], want[1]), (device, int(np.count_nonzero(got[1] != want[1])))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_any_op_on_a_three_channel_file_is_op_zero(enc, afiles, layout):  # noqa: F811
    """GUARANTEE 3: the 3-channel file into three and four planes (the fourth: 255) under every op, against the same call with
    records without an op"""
    kinds = PLANAR_KINDS if layout == "planar" else HWC_KINDS
    for c in (3, 4):
        plan = [(c, [(WHOLE90, full, w, VM.FILTERS[k % 2], bool(k & 1), kinds[k % len(kinds)]) for k, (full, w) in enumerate(((UP90, W65), (UP90, W130), (DOWN90, D64), (DOWN90, None)))])]
        want = _decode(enc, layout, [afiles.pngs[RGB90]], plan, "float32", c == 4, [[NONE] * 4])
        for ops in ([PRE, WHITE, TEAL, PRE], [ROSE, PRE, PRE, BLACK]):
            got = _decode(enc, layout, [afiles.pngs[RGB90]], plan, "float32", c == 4, [ops])
            assert got[0][0][0] == want[0][0][0] == 0 and not (want[1] == want[1][0]).all() and np.array_equal(got[1], want[1]), (c, ops)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_a_view_does_not_depend_on_the_files_other_views(enc, afiles, amodel, layout):  # noqa: F811
    """GUARANTEE 4: the views of the 90 x 40 file in the opposite order, and four of them as the file's only view (a premultiplied
    view into three planes alone: the job decodes four planes for it): the same elements, all against the model"""
    idx, plan, alpha = _alpha_plan(layout, 1)
    c, views = plan[0]
    _run(enc, afiles, amodel, layout, [idx[0]], [(c, views[::-1])], "float16", True, [alpha[0][::-1]])
    for k in (1, 4, 9, 18):
        for cc in (3, 4):
            _run(enc, afiles, amodel, layout, [idx[0]], [(cc, [views[k]])], "uint8", False, [[alpha[0][k]]])


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_a_damaged_file_leaves_the_others_views_unchanged(enc, afiles, amodel, layout, device):  # noqa: F811
    """a damaged file with alpha records between good ones: its status is the plain views call's, nothing of its destinations is
    written, and every view of every other file is exact"""
    import torch
    kinds = PLANAR_KINDS if layout == "planar" else HWC_KINDS
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
    idx, plan, alpha = _alpha_plan(layout, int(device))
    plan.insert(1, (3, damaged[1]))
    alpha.insert(1, [PRE, WHITE])
    pngs = [afiles.pngs[idx[0]], damaged[0]] + [afiles.pngs[i] for i in idx[1:]]
    got, host, outs, regs = _decode(enc, layout, pngs, plan, "uint8", device, alpha)
    assert [st for st, _, _ in got] == [0, damaged[2]] + [0] * (len(idx) - 1) and got[1][1] is None
    diff = _difference(layout, host, "uint8", regs, _sources(amodel, [idx[0], None] + idx[1:], plan, "uint8", alpha, skip=(1,)))
    assert diff is None, diff


def test_a_descriptor_carries_its_records_and_decodes_again(enc, afiles, amodel):  # noqa: F811
    """make_decode_batch_views(..., alpha=) once, decoded twice over overwritten outputs: the same both times; alpha= next to a
    descriptor is refused"""
    import torch
    import fpng_amd
    idx, plan, alpha = _alpha_plan("planar", 0)
    dev = _device_files([afiles.pngs[i] for i in idx], shift=2)
    outs = [[torch.zeros((c,) + _window(full, window)[:1:-1], dtype=torch.float32, device="cuda") for _, full, window, *_ in views] for c, views in plan]
    nest = [[[v[k] for v in views] for _, views in plan] for k in range(5)]
    db = enc.make_decode_batch_views(dev, nest[0], outs, nest[1], nest[2], nest[3], mirror=nest[4], scale=CONSTS[0][0], bias=CONSTS[0][1], alpha=_alpha_records(alpha))
    want = _sources(amodel, idx, plan, "float32", alpha)
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
        enc.decode_device_views(db, alpha=fpng_amd.view_alpha("premultiplied"))
