"""GPU decoder of several resized views of each file THROUGH A PER-VIEW AFFINE WARP (-m gpu;
fpng_amd_decode_batch(_device)_planar_views_warp and _hwc_views_warp: the post call, and for a view with a warp flag
dec_view_post_kernel's gather -- every sample that the post stage would load from the un-mirrored uint8 window in the scratch, the
blur's reflected halo included, is instead the warp's nearest byte or its blend of four): planar and channels-last destinations,
uint8 and the three float dtypes, three and four channels, both warp filters, mirrors, host and device files, with and without
blur, point operations and matrices, warp and non-warp views mixed in one file.

Expected values never come from the library: the bytes are the REFERENCE's decoder's, resized by resize_view_model.py, coloured by
color_model.py, warped by warp_model.py and post-processed by post_model.py (exact restatements; test_views_warp_cpu.py holds
warp_model against the host twin and Pillow).  The guarantee tests alone compare calls of the library with each other, as the
guarantees say.  Every call decodes into ONE sentinel-filled buffer that is compared WHOLE and bit for bit.

A warp record here is warp_model's dict: {"a": six coefficients, "filter": "nearest" | "bilinear", "fill": four bytes}, {} for a view
without a warp; a post record is post_model's dict."""
import numpy as np
import pytest

from test_gpu_decode import UNDECIDED, _device_files
from test_gpu_decode_float import CONSTS
from test_gpu_decode_layouts import SENTINEL, _damaged_files, _header_dims
from test_gpu_decode_planar import KINDS as PLANAR_KINDS, _Region as _PlanarRegion
from test_gpu_decode_resize import BITS, DTYPES, ELEM, enc, files  # noqa: F401  (enc, files: fixtures)
from test_gpu_decode_views_color import LAYOUTS, _difference, _matrices
from test_gpu_decode_views_hwc import KINDS as HWC_KINDS, _Region as _HwcRegion
from test_gpu_decode_views_post import _decode as _post_decode, _records as _post_records, _windows_plan
from test_gpu_resize_view import _window, model  # noqa: F401  (model: a fixture)
import resize_view_model as VM
import warp_model as WM

pytestmark = pytest.mark.gpu

# the windows, at tile edges only (tiles are 64 x 16): one past a tile each way, exactly one tile, three columns and rows of tiles
# with the last of each partial, and a window smaller than anything
W65, W64, W130, W3 = (30, 3, 65, 17), (10, 5, 64, 16), (100, 20, 130, 33), (7, 7, 3, 2)


def _warp_records(warp):
    import fpng_amd
    return [[fpng_amd.view_warp(p["a"], p["filter"], p["fill"]) if p else fpng_amd.view_warp() for p in ps] for ps in warp]


def _decode(enc, layout, pngs, plan, dtype, device, color, post, warp, dev=None, consts=CONSTS[0]):  # noqa: F811
    """test_gpu_decode_views_post's _decode with warp= (per file a list of a warp record per view; post None: no post= at all): ONE
    call into ONE sentinel-filled buffer -> (results, the buffer afterwards, the tensors, the regions in the records' order)"""
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


def _sources(model, idx, plan, dtype, color, post, warp, skip=(), consts=CONSTS[0]):  # noqa: F811
    """the (oh, ow, c) element bits of every view under its matrix (color None: the identity), warp and post record (post None: no
    flags), in the records' order (None for the views of the files in `skip`)"""
    return [None if n in skip else WM.view_elements(model.view(idx[n], crop, full, window, f), c, dtype, m, None if color is None else color[n][k], consts,
                                                    {} if post is None else post[n][k], warp[n][k])
            for n, (c, views) in enumerate(plan) for k, (crop, full, window, f, m, _) in enumerate(views)]


def _run(enc, files, model, layout, idx, plan, dtype, device, color, post, warp, **kw):  # noqa: F811
    got, host, outs, regs = _decode(enc, layout, [files.pngs[i] for i in idx], plan, dtype, device, color, post, warp, **kw)
    assert len(got) == len(idx)
    for n, (i, (st, views, cf)) in enumerate(zip(idx, got)):
        assert st == 0 and cf == files.chans[i] and len(views) == len(outs[n]) and all(a is b for a, b in zip(views, outs[n])), (n, i, st, cf)
    diff = _difference(layout, host, dtype, regs, _sources(model, idx, plan, dtype, color, post, warp, consts=kw.get("consts", CONSTS[0])))
    assert diff is None, (layout, dtype, device, diff)


def _matrix(window, **kw):
    import fpng_amd
    return fpng_amd.affine_matrix(window[2], window[3], **kw)


def _warp_plan(files, layout, filter, k0):  # noqa: F811
    """counts 1, 10, 1: a 1 x 1 file under a warp, a 4-channel 600 x 130 file (k0 odd: the `noise` one) with ten views -- both warp
    filters on every window, alone, in front of a blur of R = 16 and R = 1 (the halo's reflected samples go through the gather), in
    front of solarize and posterize; a rotation of a single tile and of the nine-tile window that leaves fill in every corner; a
    translation wholly outside (all fill, and the fill solarized); a post view without a warp and a direct view between them --
    and a 3-channel 600 x 130 file whose fourth plane, when it has one, is warped 255 with fill[3].  k0 flips every mirror flag and
    swaps three and four channels"""
    flip = bool(k0 & 1)
    kinds = PLANAR_KINDS if layout == "planar" else HWC_KINDS
    i600, whole, full = (5 if flip else 4), (0, 0, 600, 130), (300, 65)
    assert files.dims[i600] == (600, 130) and files.chans[i600] == 4 and files.dims[14 + flip] == (1, 1) and files.dims[2] == (600, 130) and files.chans[2] == 3
    near, lin = "nearest", "bilinear"
    views = [(W130, False, {}, {"a": _matrix(W130, angle=30.0), "filter": near, "fill": (10, 20, 30, 40)}),
             (W130, True, {"blur": (16, 5.0)}, {"a": _matrix(W130, angle=-20.0, scale=1.2), "filter": lin, "fill": (255, 0, 128, 7)}),
             (W65, True, {"blur": (1, 0.5), "solarize": 100}, {"a": [1.0, 0.37, -2.5, 0.0, 1.0, 0.0], "filter": near, "fill": (0, 0, 0, 0)}),
             (W65, False, {"solarize": 128, "posterize": 5}, {"a": _matrix(W65, angle=10.0, translate=(2.5, -1.25)), "filter": lin, "fill": (200, 100, 50, 25)}),
             (W64, False, {}, {"a": _matrix(W64, angle=45.0), "filter": near, "fill": (1, 2, 3, 4)}),
             (W64, True, {"solarize": 90}, {"a": [1.0, 0.0, -100.0, 0.0, 1.0, 0.0], "filter": lin, "fill": (99, 80, 250, 128)}),
             (W3, False, {"blur": (1, 2.0)}, {"a": _matrix(W3, angle=37.0), "filter": near, "fill": (77, 66, 55, 44)}),
             (W3, True, {}, {"a": [1.0, 0.0, 0.5, 0.0, 1.0, 0.5], "filter": lin, "fill": (9, 8, 7, 6)}),
             (W130, False, {"blur": (11, 1.3), "posterize": 3}, {}),
             (W65, True, {}, {})]
    idx = [14 + flip, i600, 2]
    plan = [(3 + flip, [((0, 0, 1, 1), (1, 1), None, filter, flip, kinds[k0 % len(kinds)])]),
            (4 - flip, [(whole, full, w, filter, m ^ flip, kinds[(k0 + k) % len(kinds)]) for k, (w, m, _, _) in enumerate(views)]),
            (3 + flip, [(whole, full, W65, filter, not flip, kinds[(k0 + 2) % len(kinds)])])]
    post = [[{}], [p for _, _, p, _ in views], [{"blur": (16, 2.0)}]]
    warp = [[{"a": [1.0, 0.0, 0.25, 0.0, 1.0, -0.25], "filter": near if flip else lin, "fill": (5, 6, 7, 8)}], [w for _, _, _, w in views],
            [{"a": [1.0, 0.0, 0.0, -0.21, 1.0, 1.75], "filter": lin if flip else near, "fill": (3, 33, 133, 233)}]]
    assert [len(v) for _, v in plan] == [1, 10, 1]
    return idx, plan, post, warp


# ---- 1. every element against the model ----
@pytest.mark.parametrize("dtype", ["uint8", "float"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_window_filter_and_post_mixed_with_views_without_warp(enc, files, model, layout, dtype):  # noqa: F811
    """the batch of _warp_plan plain and flipped: uint8 and one float dtype per layout, bilinear and bicubic resizes, a matrix per
    view and NULL colours, host and device files, dealt so that each value of each meets both values of the others"""
    dtype = "uint8" if dtype == "uint8" else ("float16" if layout == "planar" else "float32")
    d = (dtype != "uint8") + LAYOUTS.index(layout)
    for k0 in (0, 1):
        idx, plan, post, warp = _warp_plan(files, layout, VM.FILTERS[(k0 + d) % 2], k0)
        # (the corners of the rotated windows and all of the translated one are fill: the plan does what its text says)
        full130 = WM.apply_plane(warp[1][0], np.zeros((33, 130), np.uint8), False, 1)
        tile = WM.apply_plane(warp[1][4], np.zeros((16, 64), np.uint8), False, 1)
        assert all(p[q, i] == 1 for p in (full130, tile) for q in (0, -1) for i in (0, -1)) and not full130.all() and not tile.all()
        assert WM.apply_plane(warp[1][5], np.zeros((16, 64), np.uint8), False, 1).all()
        color = _matrices(plan, 80 + k0) if (k0 + d // 2) % 2 == 0 else None
        _run(enc, files, model, layout, idx, plan, dtype, bool((k0 + d + d // 2) & 1), color, post, warp, consts=CONSTS[k0])


@pytest.mark.parametrize("dtype", [t for t in DTYPES if t != "uint8"])
def test_the_other_dtypes_on_one_shape(enc, files, model, dtype):  # noqa: F811
    """every float dtype in both layouts on the 65 x 17 window: both warp filters, mirrored and not, with and without posts (NULL
    posts: the call's own records without flags)"""
    for layout in LAYOUTS:
        kinds = PLANAR_KINDS if layout == "planar" else HWC_KINDS
        whole, full = (0, 0, 600, 130), (300, 65)
        plan = [(4, [(whole, full, W65, "bilinear", bool(k & 1), kinds[k % len(kinds)]) for k in range(3)]), (4, [(whole, full, W65, "bicubic", True, kinds[-1])])]
        warp = [[{"a": _matrix(W65, angle=-15.0, shear=(8.0, 0.0)), "filter": "bilinear", "fill": (1, 128, 255, 64)}, {},
                 {"a": _matrix(W65, angle=15.0, scale=0.8), "filter": "nearest", "fill": (250, 5, 90, 0)}],
                [{"a": [1.0, 0.0, 3.0, 0.0, 1.0, -2.0], "filter": "bilinear", "fill": (0, 255, 0, 255)}]]
        post = [[{"blur": (2, 1.0)}, {"posterize": 4}, {}], [{"solarize": 77}]]
        for posts in (post, None):
            _run(enc, files, model, layout, [4, 2], plan, dtype, posts is None, None if posts is None else _matrices(plan, 90), posts, warp)


# ---- 2. the guarantees: calls against each other ----
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_records_without_flags_and_the_identity_are_the_post_call(enc, files, layout, dtype):  # noqa: F811
    """GUARANTEES 1 and 2 on the post test's batch of windows (counts 1, 10, 2, 1; blurs of every radius, point operations, direct
    views, mirrors, three and four channels): the buffer after the warp call with records of flags 0, and with the identity under
    the nearest and the bilinear filter on every view (fills that would show), equals the buffer after the post call, whole and bit
    for bit -- with matrices and with NULL colours, host and device files"""
    for device in (True, False):
        idx, plan, post = _windows_plan(files, layout, VM.FILTERS[device], int(device))
        pngs = [files.pngs[i] for i in idx]
        dev = _device_files(pngs, shift=1) if device else None
        for color in (_matrices(plan, 70 + device), None):
            want = _post_decode(enc, layout, pngs, plan, dtype, device, color, post, dev=dev)
            assert not (want[1] == want[1][0]).all()  # (something was written)
            none = [[{}] * len(views) for _, views in plan]
            ident = [[{"a": WM.IDENTITY, "filter": ("nearest", "bilinear")[(n + k) & 1], "fill": (1, 2, 3, 4)} for k in range(len(views))] for n, (_, views) in enumerate(plan)]
            for name, warp in (("flags 0", none), ("identity", ident)):
                got = _decode(enc, layout, pngs, plan, dtype, device, color, post, warp, dev=dev)
                assert [(st, cf) for st, _, cf in got[0]] == [(st, cf) for st, _, cf in want[0]] == [(0, files.chans[i]) for i in idx]
                assert np.array_equal(got[1], want[1]), (name, device, color is None, int(np.count_nonzero(got[1] != want[1])))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_a_view_does_not_depend_on_the_files_other_views(enc, files, model, layout):  # noqa: F811
    """GUARANTEE 3: the ten views of the 600 x 130 file in the opposite order (other record numbers, other offsets in the scratch),
    and three of them as the file's only view: the same elements (all against the model)"""
    idx, plan, post, warp = _warp_plan(files, layout, "bicubic", 1)
    color = _matrices(plan, 81)
    c, views = plan[1]
    _run(enc, files, model, layout, [idx[1]], [(c, views[::-1])], "float16", True, [color[1][::-1]], [post[1][::-1]], [warp[1][::-1]])
    for k in (1, 4, 7):
        _run(enc, files, model, layout, [idx[1]], [(c, [views[k]])], "float16", True, [[color[1][k]]], [[post[1][k]]], [[warp[1][k]]])


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_a_damaged_file_leaves_the_others_views_unchanged(enc, files, model, layout, device):  # noqa: F811
    """a damaged file with warp records between good ones: its status is the plain views call's, nothing of its destinations is
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
    idx, plan, post, warp = _warp_plan(files, layout, "bilinear", int(device))
    plan.insert(1, (3, damaged[1]))
    post.insert(1, [{}, {"solarize": 3}])
    warp.insert(1, [{"a": [1.0, 0.1, 0.0, 0.0, 1.0, 0.0], "filter": "bilinear", "fill": (1, 1, 1, 1)}, {"a": WM.IDENTITY, "filter": "nearest", "fill": (2, 2, 2, 2)}])
    pngs = [files.pngs[idx[0]], damaged[0]] + [files.pngs[i] for i in idx[1:]]
    color = _matrices(plan, 11)
    got, host, outs, regs = _decode(enc, layout, pngs, plan, dtype, device, color, post, warp)
    assert [st for st, _, _ in got] == [0, damaged[2], 0, 0] and got[1][1] is None
    # (the damaged file's sources are None: its regions are expected to be all sentinel)
    diff = _difference(layout, host, dtype, regs, _sources(model, [idx[0], None] + idx[1:], plan, dtype, color, post, warp, skip=(1,)))
    assert diff is None, diff


def test_a_descriptor_carries_its_records_and_decodes_again(enc, files, model):  # noqa: F811
    """make_decode_batch_views(..., warp=) once, decoded twice over overwritten outputs: the same both times; warp= next to a
    descriptor is refused"""
    import torch
    import fpng_amd
    idx, plan, post, warp = _warp_plan(files, "planar", "bilinear", 0)
    dev = _device_files([files.pngs[i] for i in idx], shift=2)
    outs = [[torch.zeros((c,) + _window(full, window)[:1:-1], dtype=torch.float32, device="cuda") for _, full, window, *_ in views] for c, views in plan]
    nest = [[[v[k] for v in views] for _, views in plan] for k in range(5)]
    db = enc.make_decode_batch_views(dev, nest[0], outs, nest[1], nest[2], nest[3], mirror=nest[4], scale=CONSTS[0][0], bias=CONSTS[0][1], post=_post_records(post),
                                     warp=_warp_records(warp))
    want = _sources(model, idx, plan, "float32", None, post, warp)
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
        enc.decode_device_views(db, warp=fpng_amd.view_warp(WM.IDENTITY))
