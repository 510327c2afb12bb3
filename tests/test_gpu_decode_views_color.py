"""GPU decoder of several resized views of each file THROUGH A PER-VIEW COLOUR MATRIX (-m gpu;
fpng_amd_decode_batch(_device)_planar_views_color and _hwc_views_color: the views call's crop stage, then dec_resize_color_kernel --
one workgroup per tile, all planes, the view's 3 x 4 matrix between the resize's bytes and the stored element): planar and
channels-last destinations, uint8 and the three float dtypes, three and four channels, both filters, mirrors, every destination
kind, host and device files.

Expected values never come from the library: the bytes are the REFERENCE's decoder's (judge()), sliced to each view's crop, resized
WHOLE and sliced to the window by resize_view_model.py; color_model.py (an exact restatement of the rule; test_views_color_cpu.py
holds it against its integer text and the host twin) turns them into elements.  The identity test alone compares two calls of the
library, as the guarantee it checks says.  Every call decodes into ONE sentinel-filled buffer that is compared WHOLE and bit for bit.

The shapes are the views tests': 600 x 130, 257 x 49, 64 x 97 and 1 x 1 files, counts 1, 10, 2, 1 in one batch (fourteen records:
the launch's prefix sums have more than one entry, and the matrices differ from record to record), and the 129 x 33 window of
three tile columns and rows with partial last tiles, plain and mirrored."""
import numpy as np
import pytest

from test_gpu_decode import UNDECIDED, _device_files
from test_gpu_decode_float import CONSTS
from test_gpu_decode_layouts import SENTINEL, _damaged_files, _header_dims
from test_gpu_decode_planar import KINDS as PLANAR_KINDS, _Region as _PlanarRegion
from test_gpu_decode_resize import BITS, CROP_OUTSIDE, DTYPES, ELEM, _expect as _planar_expect, _first_difference as _planar_difference, enc, files  # noqa: F401  (enc, files: fixtures)
from test_gpu_decode_views import _all_views as _planar_views, _mixed_counts
from test_gpu_decode_views_hwc import KINDS as HWC_KINDS, _all_views as _hwc_views, _expect as _hwc_expect, _first_difference as _hwc_difference, _hwc_kinds, _Region as _HwcRegion
from test_gpu_resize_view import _window, model  # noqa: F401  (model: a fixture)
import color_model as CM
import resize_view_model as VM
from test_views_color_cpu import CLAMP_GAIN, CLAMP_MIX, IDENTITY, TIES

pytestmark = pytest.mark.gpu

LAYOUTS = ["planar", "hwc"]


def _decode(enc, layout, pngs, plan, dtype, device, color, dev=None, consts=CONSTS[0]):  # noqa: F811
    """plan: per file (c, [(crop, full, window, filter, mirror, kind)]); color: None (the plain call), or per file a list of a
    matrix per view.  ONE call into ONE sentinel-filled buffer: (results, the buffer afterwards -- element bits for planar
    destinations, bytes for channels-last ones, as the two regions' classes count -- and the regions in the records' order)"""
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


def _sources(model, idx, plan, dtype, color, skip=(), consts=CONSTS[0]):  # noqa: F811
    """the (oh, ow, c) element bits of every view under its matrix, in the records' order (None for the views of the files in `skip`)"""
    return [None if n in skip else CM.view_elements(model.view(idx[n], crop, full, window, f), c, dtype, m, color[n][k], consts)
            for n, (c, views) in enumerate(plan) for k, (crop, full, window, f, m, _) in enumerate(views)]


def _difference(layout, host, dtype, regs, sources):
    if layout == "planar":
        return _planar_difference(host, _planar_expect(host.size, dtype, regs, sources), regs)
    return _hwc_difference(host, _hwc_expect(regs, host.size, sources), regs)


def _matrices(plan, seed):
    """a different matrix for every view of every file: ColorJitter-style ones (with grayscale among them) and arbitrary ones that
    mix channels, with constants that reach both ends of the clamp"""
    import fpng_amd
    rng = np.random.default_rng(seed)
    out = []
    for _, views in plan:
        ms = []
        for _ in views:
            if rng.random() < 0.5:
                ms.append(fpng_amd.color_matrix(brightness=rng.uniform(0.6, 1.4), contrast=rng.uniform(0.6, 1.4), saturation=(0.0 if rng.random() < 0.2 else rng.uniform(0.6, 1.4)),
                                                hue=rng.uniform(-0.1, 0.1), contrast_center=rng.uniform(100.0, 150.0)))
            else:
                m = rng.uniform(-2.0, 2.0, size=(3, 4))
                m[:, 3] = rng.uniform(-200.0, 200.0, size=3)
                ms.append(m.astype(np.float32))
        out.append(ms)
    flat = [m.tobytes() for ms in out for m in ms]
    assert len(set(flat)) == len(flat)
    return out


def _run(enc, files, model, layout, idx, plan, dtype, device, color, **kw):  # noqa: F811
    got, host, outs, regs = _decode(enc, layout, [files.pngs[i] for i in idx], plan, dtype, device, color, **kw)
    assert len(got) == len(idx)
    for n, (i, (st, views, cf)) in enumerate(zip(idx, got)):
        assert st == 0 and cf == files.chans[i] and len(views) == len(outs[n]) and all(a is b for a, b in zip(views, outs[n])), (n, i, st, cf)
    diff = _difference(layout, host, dtype, regs, _sources(model, idx, plan, dtype, color, consts=kw.get("consts", CONSTS[0])))
    assert diff is None, (layout, dtype, device, diff)


def _kinds(layout, plan):
    return _hwc_kinds(plan) if layout == "hwc" else plan


# ---- 1. the identity ----
@pytest.mark.parametrize("filter", VM.FILTERS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_the_identity_is_the_plain_views_call(enc, files, layout, dtype, filter):  # noqa: F811
    """GUARANTEE 1: every other file with ALL the views of its size (mirror flags alternating, every destination kind), three and
    four channels, host and device files -- the buffer after the call with color = the identity equals the buffer after the plain
    call of the same build, whole and bit for bit"""
    idx = list(range(len(files.pngs)))[::2]
    all_views = _planar_views if layout == "planar" else _hwc_views
    for device in (True, False):
        for c in (3, 4):
            plan = [(c, all_views(files, i, filter, k0=i + c)) for i in idx]
            pngs = [files.pngs[i] for i in idx]
            dev = _device_files(pngs, shift=1) if device else None
            plain = _decode(enc, layout, pngs, plan, dtype, device, None, dev=dev)
            ident = _decode(enc, layout, pngs, plan, dtype, device, [[IDENTITY] * len(views) for _, views in plan], dev=dev)
            assert [(st, cf) for st, _, cf in plain[0]] == [(st, cf) for st, _, cf in ident[0]] == [(0, files.chans[i]) for i in idx]
            assert not (plain[1] == plain[1][0]).all()  # (something was written)
            assert np.array_equal(plain[1], ident[1]), (device, c, int(np.count_nonzero(plain[1] != ident[1])))
    # one matrix for all views is the same call
    one = _decode(enc, layout, pngs, plan, dtype, False, IDENTITY)
    assert np.array_equal(one[1], ident[1])


# ---- 2. random matrices ----
@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_a_different_matrix_for_every_view_mixed_counts(enc, files, model, layout, dtype, device):  # noqa: F811
    """counts 1, 10, 2, 1 over a stored 4-channel, a 2-pass 4-channel, a stored 3-channel and a 1-pass 3-channel file, into 4, 3, 4
    and 3 channels (alpha untouched by the matrix, dropped, A = 255 through fmaf(255, scale[3], bias[3])), every destination kind
    of the layout -- planar: reversed plane order and negative pitches among them -- both filters and mirrors in one file"""
    for k0 in (0, 3):
        idx, plan = _mixed_counts(files, k0)
        plan = _kinds(layout, plan)
        assert [files.chans[i] for i in idx] == [4, 4, 3, 3] and [c for c, _ in plan] == [4, 3, 4, 3] and sum(len(v) for _, v in plan) == 14
        kinds = {v[5] for _, views in plan for v in views}
        assert kinds >= ({"reversed", "bottom_up"} | ({"px4"} if layout == "hwc" else {"pad256"}))
        _run(enc, files, model, layout, idx, plan, dtype, device, _matrices(plan, 100 + k0), consts=CONSTS[k0 & 1])


@pytest.mark.parametrize("filter", VM.FILTERS)
@pytest.mark.parametrize("dtype", ["uint8", "float16"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_tile_borders_plain_and_mirrored(enc, files, model, layout, dtype, filter):  # noqa: F811
    """a window of 129 x 33 samples -- three tile columns and rows, the last of each partial -- plain and MIRRORED, and the 65 x 17
    and 2 x 194 windows mirrored, over every destination kind, three and four channels, every view its own matrix"""
    kinds = PLANAR_KINDS if layout == "planar" else HWC_KINDS
    whole = (0, 0, 600, 130)
    i600 = [i for i, d in enumerate(files.dims) if d == (600, 130)]
    i64 = [i for i, d in enumerate(files.dims) if d == (64, 97)]
    idx, plan = [], []
    for n, i in enumerate(i600):
        views = [(whole, (300, 65), (0, 0, 129, 33), filter, False, kinds[n % len(kinds)]), (whole, (300, 65), (0, 0, 129, 33), filter, True, kinds[(n + 1) % len(kinds)]),
                 (whole, (300, 65), (235, 48, 65, 17), filter, True, kinds[(n + 2) % len(kinds)])]
        idx.append(i), plan.append((3 + (n & 1), views))
    for n, i in enumerate(i64):
        idx.append(i), plan.append((4 - n, [((0, 0, 64, 97), (128, 194), (63, 0, 2, 194), filter, True, kinds[(2 + 3 * n) % len(kinds)])]))
    _run(enc, files, model, layout, idx, plan, dtype, True, _matrices(plan, 7))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_a_view_does_not_depend_on_the_files_other_views(enc, files, model, layout):  # noqa: F811
    """GUARANTEE 2: the ten views of a 600 x 130 file in one call, and each of them as the file's only view with the same matrix:
    the same elements (both against the model, so against each other)"""
    i = [k for k, d in enumerate(files.dims) if d == (600, 130)][1]
    views = (_planar_views if layout == "planar" else _hwc_views)(files, i, "bicubic", k0=1)
    mats = _matrices([(3, views)], 55)
    _run(enc, files, model, layout, [i], [(3, views)], "float16", True, mats)
    for k in (0, 4, 9):
        _run(enc, files, model, layout, [i], [(3, [views[k]])], "float16", True, [[mats[0][k]]])


# ---- 3. rounding and clamp on the device ----
@pytest.mark.parametrize("dtype", ["uint8", "float16"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_ties_and_both_ends_of_the_clamp(enc, files, model, layout, dtype):  # noqa: F811
    """the tie matrix (x.5 for every odd byte: rint goes to the even neighbour) and the two clamp matrices (gain 4, constant -300:
    0 up to byte 75, 255 from 139 on) on views WITHOUT a resize -- full = the crop's size, so the bytes are the file's own, `noise`
    files among them -- and on resized ones"""
    kinds = PLANAR_KINDS if layout == "planar" else HWC_KINDS
    idx = [i for i, d in enumerate(files.dims) if d in ((257, 49), (64, 97))]
    plan, color = [], []
    for n, i in enumerate(idx):
        w, h = files.dims[i]
        views = [((0, 0, w, h), (w, h), None, "bilinear", bool(n & 1), kinds[n % len(kinds)]), ((1, 1, w - 2, h - 2), (w - 2, h - 2), (0, 0, w - 2, h - 3), "bicubic", not (n & 1), kinds[(n + 1) % len(kinds)]),
                 ((0, 0, w, h), (70, 20), None, "bicubic", False, kinds[(n + 2) % len(kinds)])]
        plan.append((3 + (n & 1), views))
        color.append([(TIES, CLAMP_GAIN, CLAMP_MIX)[(n + k) % 3] for k in range(3)])
    src = _sources(model, idx, plan, "uint8", color)
    assert any((s[..., :3] == 0).any() and (s[..., :3] == 255).any() for s in src)  # (both ends of the clamp are reached)
    _run(enc, files, model, layout, idx, plan, dtype, True, color)


# ---- 4. unchanged around it ----
@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("dtype", ["uint8", "float16"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_statuses(enc, files, model, layout, dtype, device):  # noqa: F811
    """a file one of whose crops leaves the image (67) and a damaged file next to good ones: the statuses are the plain views
    call's, nothing of the two files' destinations is written, every other file is exact"""
    import torch
    kinds = PLANAR_KINDS if layout == "planar" else HWC_KINDS
    damaged = None
    for p in _damaged_files():
        w, h = _header_dims(p)
        if not (2 <= w <= 600 and 2 <= h <= 600):
            continue
        dviews = [((0, h - 2, w, 2), (max(w // 3, 1), 3), None, "bicubic", True, "odd"), ((0, 0, min(w, 5), 1), (3, 3), (1, 1, 2, 2), "bilinear", False, kinds[0])]
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
    plain = _decode(enc, layout, pngs, plan, dtype, device, None)
    got, host, outs, regs = _decode(enc, layout, pngs, plan, dtype, device, color)
    assert [(st, cf) for st, _, cf in got] == [(st, cf) for st, _, cf in plain[0]]
    assert [st for st, _, _ in got] == [0, 0, CROP_OUTSIDE, 0, damaged[2]] and got[2][1] is None and got[4][1] is None
    # (the rejected files' sources are None: their regions are expected to be all sentinel)
    diff = _difference(layout, host, dtype, regs, _sources(model, idx + [None], plan, dtype, color, skip=(2, 4)))
    assert diff is None, diff


def test_a_descriptor_carries_its_matrices_and_decodes_again(enc, files, model):  # noqa: F811
    """make_decode_batch_views(..., color=) once, decoded twice over overwritten outputs; color= next to a descriptor is refused"""
    import torch
    idx, plan = _mixed_counts(files, 0)
    dev = _device_files([files.pngs[i] for i in idx], shift=2)
    color = _matrices(plan, 3)
    outs = [[torch.zeros((c,) + _window(full, window)[:1:-1], dtype=torch.float32, device="cuda") for _, full, window, *_ in views] for c, views in plan]
    nest = [[[v[k] for v in views] for _, views in plan] for k in range(5)]
    db = enc.make_decode_batch_views(dev, nest[0], outs, nest[1], nest[2], nest[3], mirror=nest[4], scale=CONSTS[0][0], bias=CONSTS[0][1], color=color)
    want = _sources(model, idx, plan, "float32", color)
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
        enc.decode_device_views(db, color=IDENTITY)
