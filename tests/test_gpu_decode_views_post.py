"""GPU decoder of several resized views of each file THROUGH A PER-VIEW POST-PROCESSING RECORD (-m gpu;
fpng_amd_decode_batch(_device)_planar_views_post and _hwc_views_post: the colour call, and for a view with a flag
dec_resize_color_kernel's un-mirrored uint8 window in the scratch, then dec_view_post_kernel -- one workgroup per tile, the tile
and a halo of the blur's radius in LDS, two integer passes, solarize, posterize, the store): planar and channels-last destinations,
uint8 and the three float dtypes, three and four channels, both filters, mirrors, every destination kind, host and device files,
with matrices and with NULL colours, direct and post views mixed in one file.

Expected values never come from the library: the bytes are the REFERENCE's decoder's, resized by resize_view_model.py, coloured by
color_model.py and post-processed by post_model.py (exact restatements; test_views_post_cpu.py holds the last against the host twin,
Pillow and scipy).  The first test alone compares calls of the library with each other, as the guarantee it checks says.  Every call
decodes into ONE sentinel-filled buffer that is compared WHOLE and bit for bit.

A post record here is post_model's dict: {"blur": (R, sigma), "solarize": threshold, "posterize": bits}, {} for a view without flags."""
import numpy as np
import pytest

from test_gpu_decode import UNDECIDED, _device_files
from test_gpu_decode_float import CONSTS
from test_gpu_decode_layouts import SENTINEL, _damaged_files, _header_dims
from test_gpu_decode_planar import KINDS as PLANAR_KINDS, _Region as _PlanarRegion
from test_gpu_decode_resize import BITS, CROP_OUTSIDE, DTYPES, ELEM, enc, files  # noqa: F401  (enc, files: fixtures)
from test_gpu_decode_views import _mixed_counts, big_files  # noqa: F401  (big_files: a fixture)
from test_gpu_decode_views_color import LAYOUTS, _decode as _color_decode, _difference, _kinds, _matrices
from test_gpu_decode_views_hwc import KINDS as HWC_KINDS, _Region as _HwcRegion
from test_gpu_resize_view import _Model, _window, model  # noqa: F401  (model: a fixture)
import post_model as PM
import resize_view_model as VM

pytestmark = pytest.mark.gpu


def _records(post):
    import fpng_amd
    return [[fpng_amd.view_post(blur=(2 * p["blur"][0] + 1, p["blur"][1]) if "blur" in p else None, solarize=p.get("solarize"), posterize=p.get("posterize")) for p in ps]
            for ps in post]


def _decode(enc, layout, pngs, plan, dtype, device, color, post, dev=None, consts=CONSTS[0]):  # noqa: F811
    """test_gpu_decode_views_color's _decode with post= (per file a list of a post record per view): ONE call into ONE
    sentinel-filled buffer -> (results, the buffer afterwards, the tensors, the regions in the records' order)"""
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
    kw["post"] = _records(post)
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


def _sources(model, idx, plan, dtype, color, post, skip=(), consts=CONSTS[0]):  # noqa: F811
    """the (oh, ow, c) element bits of every view under its matrix (color None: the identity) and post record, in the records'
    order (None for the views of the files in `skip`)"""
    return [None if n in skip else PM.view_elements(model.view(idx[n], crop, full, window, f), c, dtype, m, None if color is None else color[n][k], consts, post[n][k])
            for n, (c, views) in enumerate(plan) for k, (crop, full, window, f, m, _) in enumerate(views)]


def _run(enc, files, model, layout, idx, plan, dtype, device, color, post, **kw):  # noqa: F811
    got, host, outs, regs = _decode(enc, layout, [files.pngs[i] for i in idx], plan, dtype, device, color, post, **kw)
    assert len(got) == len(idx)
    for n, (i, (st, views, cf)) in enumerate(zip(idx, got)):
        assert st == 0 and cf == files.chans[i] and len(views) == len(outs[n]) and all(a is b for a, b in zip(views, outs[n])), (n, i, st, cf)
    diff = _difference(layout, host, dtype, regs, _sources(model, idx, plan, dtype, color, post, consts=kw.get("consts", CONSTS[0])))
    assert diff is None, (layout, dtype, device, diff)


# ---- 1. records without flags ----
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_records_without_flags_are_the_colour_call_and_the_plain_call(enc, files, layout, dtype):  # noqa: F811
    """GUARANTEE 1: counts 1, 10, 2, 1, both filters, mirrors, every destination kind, three and four channels, host and device
    files -- the buffer after the post call with records of flags 0 equals the buffer after the colour call with the same
    matrices, and with NULL colours the buffer after the plain call, whole and bit for bit"""
    for device in (True, False):
        idx, plan = _mixed_counts(files, 1 + device)
        plan = _kinds(layout, plan)
        pngs = [files.pngs[i] for i in idx]
        dev = _device_files(pngs, shift=1) if device else None
        color = _matrices(plan, 40 + device)
        none = [[{}] * len(views) for _, views in plan]
        plain = _color_decode(enc, layout, pngs, plan, dtype, device, None, dev=dev)
        coloured = _color_decode(enc, layout, pngs, plan, dtype, device, color, dev=dev)
        assert not (plain[1] == plain[1][0]).all() and not np.array_equal(plain[1], coloured[1])  # (something was written, and the matrices matter)
        for want, col in ((plain, None), (coloured, color)):
            got = _decode(enc, layout, pngs, plan, dtype, device, col, none, dev=dev)
            assert [(st, cf) for st, _, cf in got[0]] == [(st, cf) for st, _, cf in want[0]] == [(0, files.chans[i]) for i in idx]
            assert np.array_equal(got[1], want[1]), (device, col is None, int(np.count_nonzero(got[1] != want[1])))


# ---- 2. every element against the model ----
def _windows_plan(files, layout, filter, k0):  # noqa: F811
    """counts 1, 10, 2, 1: a 1 x 1 file (flags 0, or point operations only), a 4-channel 600 x 130 file (k0 odd: the `noise` one) with
    the blur's windows -- 129 x 33 (three tile columns and rows, the last of each partial) at R = 16 and R = 1, 17 x 17 at R = 16
    (the reflection reaches the far edge from both sides), 64 x 16 (one tile) and 65 x 17 at R = 11, 2 x 2 at R = 1 -- between direct
    views and a point-only one, the 4-channel `noise` 64 x 97 file unresized (seven tile rows) next to a direct view of it, and a
    257 x 49 file into exactly one tile.  k0 flips every mirror flag and swaps three and four channels; every record differs"""
    flip = bool(k0 & 1)
    kinds = PLANAR_KINDS if layout == "planar" else HWC_KINDS
    i600, whole, full = (5 if flip else 4), (0, 0, 600, 130), (300, 65)
    assert files.dims[i600] == (600, 130) and files.chans[i600] == 4 and files.dims[14 + flip] == (1, 1) and files.dims[13] == (64, 97) and files.dims[6 + 3 * flip] == (257, 49)
    wins = [((0, 0, 129, 33), False, {"blur": (16, 5.0)}),
            ((0, 0, 129, 33), True, {"blur": (1, 0.5), "solarize": 100}),
            ((100, 20, 17, 17), True, {"blur": (16, 2.0)}),
            ((10, 5, 64, 16), False, {"blur": (11, 1.3), "posterize": 3}),
            ((0, 0, 129, 33), False, {}),
            ((235, 48, 65, 17), True, {"blur": (11, 2.0), "solarize": 128, "posterize": 5}),
            ((7, 7, 2, 2), False, {"blur": (1, 2.0)}),
            ((171, 32, 129, 33), True, {"solarize": 128}),
            ((30, 3, 65, 17), True, {}),
            ((0, 0, 129, 33), True, {"blur": (16, 1.3), "posterize": 7})]
    idx = [14 + flip, i600, 13, 6 + 3 * flip]
    plan = [(3 + flip, [((0, 0, 1, 1), (1, 1), None, filter, flip, kinds[k0 % len(kinds)])]),
            (4 - flip, [(whole, full, w, filter, m ^ flip, kinds[(k0 + k) % len(kinds)]) for k, (w, m, _) in enumerate(wins)]),
            (3 + flip, [((0, 0, 64, 97), (64, 97), None, filter, flip, kinds[(k0 + 2) % len(kinds)]), ((7, 5, 50, 90), (128, 6), None, filter, not flip, kinds[(k0 + 3) % len(kinds)])]),
            (4 - flip, [((1, 1, 255, 47), (64, 16), None, filter, not flip, kinds[(k0 + 4) % len(kinds)])])]
    post = [[{} if flip else {"solarize": 0, "posterize": 3}], [p for _, _, p in wins], [{"blur": (16, 0.5 + k0), "solarize": 200}, {}], [{"blur": (11, 0.1 + k0)}]]
    flat = [repr(sorted(p.items())) for ps in post for p in ps if p]
    assert len(set(flat)) == len(flat) and [len(v) for _, v in plan] == [1, 10, 2, 1]
    return idx, plan, post


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_window_and_radius_mixed_with_direct_views(enc, files, model, layout, dtype):  # noqa: F811
    """the batch of _windows_plan plain and flipped: bilinear and bicubic, a matrix per view and NULL colours, host and device files,
    dealt over the dtypes and layouts so that each value of each meets both values of the others"""
    d = DTYPES.index(dtype) + LAYOUTS.index(layout)
    for k0 in (0, 1):
        idx, plan, post = _windows_plan(files, layout, VM.FILTERS[(k0 + d) % 2], k0)
        color = _matrices(plan, 60 + k0) if (k0 + d // 2) % 2 == 0 else None
        _run(enc, files, model, layout, idx, plan, dtype, bool((k0 + d + d // 2) & 1), color, post, consts=CONSTS[k0])


@pytest.mark.parametrize("layout", LAYOUTS)
def test_a_view_does_not_depend_on_the_files_other_views(enc, files, model, layout):  # noqa: F811
    """GUARANTEE 2: the ten views of the 600 x 130 file in the opposite order (the direct and the post launches see other record
    numbers, the scratch other offsets), and three of them as the file's only view: the same elements (all against the model)"""
    idx, plan, post = _windows_plan(files, layout, "bicubic", 1)
    color = _matrices(plan, 61)
    c, views = plan[1]
    _run(enc, files, model, layout, [idx[1]], [(c, views[::-1])], "float16", True, [color[1][::-1]], [post[1][::-1]])
    for k in (0, 4, 5):
        _run(enc, files, model, layout, [idx[1]], [(c, [views[k]])], "float16", True, [[color[1][k]]], [[post[1][k]]])


def test_more_than_one_group(enc, big_files):  # noqa: F811
    """post and direct views of three large host files: every group launches its own jobs' ranges of both kinds of records"""
    plan = [(3, [((1000, 1000, 24, 24), (12, 12), None, "bilinear", False, "packed"), ((3, 5, 40, 30), (20, 15), (2, 2, 8, 8), "bicubic", True, "odd")]),
            (4, [((500, 700, 64, 16), (8, 2), None, "bicubic", True, "reversed")]),
            (3, [((0, 0, 9, 9), (27, 27), (20, 20, 7, 7), "bicubic", False, "bottom_up"), ((1015, 0, 9, 1024), (3, 32), None, "bilinear", True, "pad256"),
                 ((512, 512, 16, 16), (16, 16), (0, 0, 16, 1), "bilinear", False, "packed")])]
    post = [[{"blur": (3, 1.0)}, {}], [{"blur": (1, 0.7), "solarize": 90}], [{}, {"blur": (2, 2.0)}, {"posterize": 2}]]
    _run(enc, big_files, _Model(big_files), "planar", [0, 1, 2], plan, "float16", False, _matrices(plan, 5), post)


# ---- 3. point operations only ----
@pytest.mark.parametrize("dtype", ["uint8", "bfloat16"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_point_operations_only(enc, files, model, layout, dtype):  # noqa: F811
    """no blur: the kernel reads the scratch straight into its registers.  Solarize thresholds 0 (everything inverted) and 255,
    posterize bits 0 (everything 0) and 8 (the identity), alone and together, on the 129 x 33 window, plain and mirrored"""
    kinds = PLANAR_KINDS if layout == "planar" else HWC_KINDS
    posts = [{"solarize": 0}, {"solarize": 255}, {"posterize": 0}, {"posterize": 8}, {"solarize": 0, "posterize": 8}, {"solarize": 255, "posterize": 1}]
    idx, plan, post = [], [], []
    for n, i in enumerate(k for k, d in enumerate(files.dims) if d == (600, 130)):
        if n % 3 == 1:
            continue
        views = [((0, 0, 600, 130), (300, 65), (0, 0, 129, 33), VM.FILTERS[n & 1], bool((n + k) & 1), kinds[(n + k) % len(kinds)]) for k in range(3)]
        idx.append(i), plan.append((3 + (n & 1), views)), post.append([posts[(n + 2 * k) % len(posts)] for k in range(3)])
    assert {repr(p) for ps in post for p in ps} == {repr(p) for p in posts}
    _run(enc, files, model, layout, idx, plan, dtype, True, _matrices(plan, 8) if dtype == "uint8" else None, post)


# ---- 4. unchanged around it ----
@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_statuses(enc, files, model, layout, device):  # noqa: F811
    """a file one of whose crops leaves the image (67) and a damaged file next to good ones, post records on all of them: the
    statuses are the plain views call's, nothing of the two files' destinations is written, every other file is exact"""
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
    idx, plan = _mixed_counts(files, 1)
    plan = _kinds(layout, plan)
    outside = [plan[2][1][0], ((files.dims[2][0] - 1, 0, 2, 1), (7, 5), (1, 1, 5, 3), "bicubic", False, "pad256"), plan[2][1][1]]
    plan[2] = (plan[2][0], outside)
    plan.append((3, damaged[1]))
    pngs = [files.pngs[i] for i in idx] + [damaged[0]]
    color = _matrices(plan, 9)
    post = []
    for n, (_, views) in enumerate(plan):  # (a blur where the window takes one, else a point operation; every third view direct)
        ps = []
        for k, (_, full, window, *_) in enumerate(views):
            w, h = _window(full, window)[2:]
            r = min(w, h, 12) - 1
            ps.append({} if (n + k) % 3 == 2 else {"blur": (r, 0.4 + 0.3 * k + n), "solarize": (30 * k + n) % 256} if r >= 1 else {"posterize": 1 + (n + k) % 7})
        post.append(ps)
    assert any("blur" in p for p in post[2]) and any("blur" in p for p in post[4])
    plain = _color_decode(enc, layout, pngs, plan, dtype, device, None)
    got, host, outs, regs = _decode(enc, layout, pngs, plan, dtype, device, color, post)
    assert [(st, cf) for st, _, cf in got] == [(st, cf) for st, _, cf in plain[0]]
    assert [st for st, _, _ in got] == [0, 0, CROP_OUTSIDE, 0, damaged[2]] and got[2][1] is None and got[4][1] is None
    # (the rejected files' sources are None: their regions are expected to be all sentinel)
    diff = _difference(layout, host, dtype, regs, _sources(model, idx + [None], plan, dtype, color, post, skip=(2, 4)))
    assert diff is None, diff


def test_a_descriptor_carries_its_records_and_decodes_again(enc, files, model):  # noqa: F811
    """make_decode_batch_views(..., post=) once, decoded twice over overwritten outputs: the same both times; post= next to a
    descriptor is refused"""
    import torch
    import fpng_amd
    idx, plan, post = _windows_plan(files, "planar", "bilinear", 0)
    dev = _device_files([files.pngs[i] for i in idx], shift=2)
    color = _matrices(plan, 3)
    outs = [[torch.zeros((c,) + _window(full, window)[:1:-1], dtype=torch.float32, device="cuda") for _, full, window, *_ in views] for c, views in plan]
    nest = [[[v[k] for v in views] for _, views in plan] for k in range(5)]
    db = enc.make_decode_batch_views(dev, nest[0], outs, nest[1], nest[2], nest[3], mirror=nest[4], scale=CONSTS[0][0], bias=CONSTS[0][1], color=color, post=_records(post))
    want = _sources(model, idx, plan, "float32", color, post)
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
        enc.decode_device_views(db, post=fpng_amd.view_post(solarize=1))
