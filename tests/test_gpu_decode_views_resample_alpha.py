"""GPU decoder of views under a PREMULTIPLIED alpha record AND a RESAMPLE filter (-m gpu; the _views_resample calls with alpha=:
the <..., kAlpha = true, kResample = true> instantiations of dec_resize_exact_kernel, dec_resize_hwc_kernel and
dec_resize_color_kernel -- the premultiply in the load of the horizontal pass, four planes through the tile whatever the destination
has, the division in the store of the vertical pass in front of the matrix; a planar call with a PREMULTIPLIED view runs the colour
kernel under identity matrices, one with composites alone the per-plane kernel): the alpha test's windows under box, Hamming and Lanczos with PREMULTIPLIED, a COMPOSITE and no op
interleaved in each file, three and four planes, both layouts, uint8 and a float dtype; the 1 x 1 files; each filter's exact scale
limit; in front of a real matrix and of a blur; NEAREST beside PREMULTIPLIED in one file.

Lanczos is the filter under which U's clip is most alive; box and Hamming have no negative weight and never clip.  Both facts are
asserted on the reference decoder's planes before the GPU is asked, so a change of the pattern cannot silently empty the test.

Expected values never come from the library: the bytes are the REFERENCE's decoder's, through resample_model.py, alpha_model.py and
enhance_model.py.  Every call decodes into ONE sentinel-filled buffer that is compared WHOLE and bit for bit."""
import numpy as np
import pytest

from test_gpu_decode import _device_files
from test_gpu_decode_float import CONSTS
from test_gpu_decode_layouts import SENTINEL
from test_gpu_decode_planar import KINDS as PLANAR_KINDS, _Region as _PlanarRegion
from test_gpu_decode_resize import BITS, ELEM, enc  # noqa: F401  (enc: a fixture)
from test_gpu_decode_views_alpha import (D1, D64, D65, DOWN90, NOISE, ONE0, ONE128, P90, P90S, PRE, ROSE, TEAL, UP90, W1, W64, W65, W130, WHITE, WHOLE90, _alpha_records, afiles,  # noqa: F401
                                         amodel)  # (afiles, amodel: fixtures)
from test_gpu_decode_views_color import LAYOUTS, _difference, _matrices
from test_gpu_decode_views_enhance import _enhance_records
from test_gpu_decode_views_hwc import KINDS as HWC_KINDS, _Region as _HwcRegion
from test_gpu_decode_views_post import _records as _post_records
from test_gpu_decode_views_resample import _names
from test_gpu_decode_views_tone import _tone_records
from test_gpu_decode_views_warp import _warp_records
from test_gpu_resize_view import _window
import resample_model as SM  # (before any model is asked for a new filter's name)
import alpha_model as AM

pytestmark = pytest.mark.gpu

NONE = {}
CONVOLUTIONS = ("box", "hamming", "lanczos")
OPS = (PRE, TEAL, NONE)
STAGES = ("alpha", "color", "post", "warp", "tone", "enhance")


def _kinds(layout):
    return PLANAR_KINDS if layout == "planar" else HWC_KINDS


def _decode(enc, layout, pngs, plan, dtype, device, alpha=None, color=None, post=None, warp=None, tone=None, enhance=None, resample=True, consts=CONSTS[0]):  # noqa: F811
    """plan: per file (c, [(crop, full, window, filter, mirror, kind)]), filter any of the six names; resample: True -- resample= from
    the plan's filters, None -- no resample= at all; alpha, color, post, warp, tone, enhance: None (the argument is not given), or per
    file a list of a record (the models' dicts; color: a matrix) per view.  ONE call into ONE sentinel-filled buffer -> (results, the
    buffer afterwards, the tensors, the regions in the records' order)"""
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
    if resample:
        kw["resample"] = [[_names(v[3])[1] for v in views] for _, views in plan]
    else:
        assert all(v[3] not in SM.NEW_FILTERS for _, views in plan for v in views)
    for name, records, make in (("alpha", alpha, _alpha_records), ("enhance", enhance, _enhance_records), ("tone", tone, _tone_records), ("warp", warp, _warp_records),
                                ("post", post, _post_records), ("color", color, lambda m: m)):
        if records is not None:
            kw[name] = make(records)
    if device:
        call = enc.decode_device_views if layout == "planar" else enc.decode_device_views_hwc
        got = call(_device_files(pngs, shift=1), *args, **kw)
    else:
        call = enc.decode_batch_views if layout == "planar" else enc.decode_batch_views_hwc
        got = call(pngs, *args, **kw)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    return got, (host.view(BITS[e]) if layout == "planar" else host), outs, regs


def _sources(model, idx, plan, dtype, alpha=None, color=None, post=None, warp=None, tone=None, enhance=None, skip=(), consts=CONSTS[0]):
    """the (oh, ow, c) element bits of every view, in the records' order (None for the views of the files in `skip`):
    alpha_model.view_elements with all ten arguments"""
    def rec(records, n, k):
        return {} if records is None else records[n][k]
    return [None if n in skip else AM.view_elements(model.view(idx[n], crop, full, window, f, rec(alpha, n, k)), c, dtype, m, None if color is None else color[n][k], consts,
                                                    rec(post, n, k), rec(warp, n, k), rec(tone, n, k), rec(enhance, n, k))
            for n, (c, views) in enumerate(plan) for k, (crop, full, window, f, m, _) in enumerate(views)]


def _run(enc, files, model, layout, idx, plan, dtype, device, consts=CONSTS[0], **stages):  # noqa: F811
    assert set(stages) <= set(STAGES)
    got, host, outs, regs = _decode(enc, layout, [files.pngs[i] for i in idx], plan, dtype, device, consts=consts, **stages)
    assert len(got) == len(idx)
    for n, (i, (st, views, cf)) in enumerate(zip(idx, got)):
        assert st == 0 and cf == files.chans[i] and len(views) == len(outs[n]) and all(a is b for a, b in zip(views, outs[n])), (n, i, st, cf)
    diff = _difference(layout, host, dtype, regs, _sources(model, idx, plan, dtype, consts=consts, **stages))
    assert diff is None, (layout, dtype, device, diff)
    return host, regs


def _clipped(r4):
    """(h, w) bool: the samples of R' (4, h, w) at which U's clip is live in some colour plane"""
    r = np.asarray(r4).astype(np.int64)
    a = r[3]
    return ((a > 0) & (a < 255))[None] & (255 * r[:3] // np.where(a == 0, 1, a) > 255)


def _check_conditions(files, pairs, filter):
    """alpha_model.conditions on the reference decoder's planes, per (file, crop, full): Lanczos clips and meets a colour under alpha
    0; box and Hamming, whose weights are not negative, do neither"""
    for i, (x, y, w, h), full in pairs:
        got = AM.conditions(files.planes[i][:, y:y + h, x:x + w], full, filter)
        if filter == "lanczos":
            assert got["clip"] >= 1 and got["zero_alpha_colour"] >= 1, (i, full, got)
        else:
            assert got["clip"] == 0 and got["zero_alpha_colour"] == 0, (filter, i, full, got)
        assert all(got[k] >= 1 for k in ("alpha_0", "alpha_255", "alpha_between")), (i, got)


def _windows_plan(layout, filter, flip):
    """the 90 x 40 pattern, compressed and stored: every window of the alpha test, upscaled and downscaled, under PREMULTIPLIED, a
    COMPOSITE and no op each, the ops interleaved; the 1 x 1 files with alpha 0 and 128 -> 5 x 5 (premultiplied: U copies, and divides
    by 128).  flip swaps three and four planes and every mirror flag; mirror flags and destination kinds are dealt round-robin.
    -> idx, plan, alpha"""
    kinds = _kinds(layout)
    views = [(full, w, OPS[(n + k) % 3]) for n, (full, w) in enumerate([(UP90, w) for w in (W1, W64, W65, W130)] + [(DOWN90, w) for w in (D1, D64, D65)]) for k in (0, 1, 2)]

    def file90(c, shift):
        return (c, [(WHOLE90, full, w, filter, flip ^ bool((k + shift) & 1), kinds[(k + shift + flip) % len(kinds)]) for k, (full, w, _) in enumerate(views)])

    ones = [((0, 0, 1, 1), (5, 5), (None, (1, 1, 3, 3), None)[k], filter, flip ^ bool(k & 1), kinds[(k + flip) % len(kinds)]) for k in range(3)]
    idx = [P90, ONE0, P90S, ONE128]
    plan = [file90(3 + flip, 0), (4 - flip, ones), file90(4 - flip, 1), (3 + flip, ones)]
    a90 = [v[2] for v in views]
    alpha = [a90, [PRE, TEAL, NONE], a90, [PRE, ROSE, PRE]]
    assert len(views) == 21 and all(a90[k:k + 3].count(op) == 1 for k in range(0, 21, 3) for op in OPS)  # (every window under every op)
    return idx, plan, alpha


# ---- 1, 2. the windows, and the conditions in front of them ----
@pytest.mark.parametrize("filter", CONVOLUTIONS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_window_premultiplied_composited_and_plain(enc, afiles, amodel, layout, filter):  # noqa: F811
    """the batch of _windows_plan: uint8 from host files, and flipped as float16 from device files"""
    _check_conditions(afiles, [(i, WHOLE90, full) for i in (P90, P90S) for full in (UP90, DOWN90)], filter)
    for flip, dtype in ((False, "uint8"), (True, "float16")):
        idx, plan, alpha = _windows_plan(layout, filter, flip)
        if filter == "lanczos":  # (some PREMULTIPLIED window of the plan holds a clipped sample, in both sizes)
            for full in (UP90, DOWN90):
                live = _clipped(AM.resized(PRE, afiles.planes[P90], full, filter)).any(axis=0)
                assert any(live[y:y + h, x:x + w].any() for _, f, (x, y, w, h), *_ in (v for v, a in zip(plan[0][1], alpha[0]) if a == PRE) if f == full), full
        _run(enc, afiles, amodel, layout, idx, plan, dtype, flip, consts=CONSTS[flip], alpha=alpha)
        if layout == "planar":  # (composites and views without an op alone: every window through the per-plane kernel's alpha and resample instantiation)
            only = [[WHITE if a == PRE else a for a in row] for row in alpha]
            _run(enc, afiles, amodel, layout, idx, plan, dtype, not flip, consts=CONSTS[flip], alpha=only)


# ---- 3. each filter's exact scale limit ----
@pytest.mark.parametrize("layout", LAYOUTS)
def test_premultiplied_at_each_filters_exact_scale_limit(enc, afiles, amodel, layout):  # noqa: F811
    """96 x 64 of the 4-channel noise file -> 3 x 2 under box and Hamming, -> 9 x 6 under Lanczos: the four-plane loop at the most
    taps, rows and LDS that resize_max_taps, resize_tile_rows and resize_tile_lds / resize_hwc_tile_lds allow, into three and four
    planes, a COMPOSITE and a view without an op beside the PREMULTIPLIED one"""
    assert afiles.dims[NOISE] == (600, 130) and afiles.chans[NOISE] == 4
    kinds = _kinds(layout)
    for filter in CONVOLUTIONS:
        full = (9, 6) if filter == "lanczos" else (3, 2)
        assert SM.scale_ok(96, full[0], filter) and not SM.scale_ok(97, full[0], filter) and SM.scale_ok(64, full[1], filter) and not SM.scale_ok(65, full[1], filter)
        for c in (3, 4):
            plan = [(c, [((0, 0, 96, 64), full, None, filter, bool((k + c) & 1), kinds[(k + c) % len(kinds)]) for k in range(3)])]
            _run(enc, afiles, amodel, layout, [NOISE], plan, "uint8", c == 4, alpha=[[PRE, TEAL, NONE]])
            _run(enc, afiles, amodel, layout, [NOISE], [(c, plan[0][1][:1])], "uint8", c == 3, alpha=[[PRE]])  # (alone: the launch's LDS is this view's)
            if layout == "planar":  # (composites alone: the per-plane kernel)
                _run(enc, afiles, amodel, layout, [NOISE], plan, "uint8", c == 3, alpha=[[ROSE, TEAL, NONE]])


# ---- 4. in front of a real matrix, in front of a blur ----
@pytest.mark.parametrize("layout", LAYOUTS)
def test_premultiplied_lanczos_in_front_of_a_matrix_and_a_blur(enc, afiles, amodel, layout):  # noqa: F811
    """the division comes first, then the matrix (a colour call); and in a post call a blur of radius 1 reads the divided window out
    of the scratch.  A COMPOSITE view and a view without an op beside the PREMULTIPLIED ones in the same file; box and Hamming
    among them"""
    _check_conditions(afiles, [(P90, WHOLE90, UP90), (P90S, WHOLE90, DOWN90)], "lanczos")
    kinds = _kinds(layout)
    shapes = [(UP90, W64, "lanczos", PRE), (UP90, W65, "lanczos", TEAL), (UP90, W130, "lanczos", NONE), (DOWN90, D65, "lanczos", PRE), (UP90, W130, "lanczos", PRE), (DOWN90, D64, "hamming", PRE),
              (UP90, W65, "box", PRE)]
    for c in (3, 4):
        plan = [(c, [(WHOLE90, full, w, f, bool((k + c) & 1), kinds[(k + c) % len(kinds)]) for k, (full, w, f, _) in enumerate(shapes)])]
        alpha = [[s[3] for s in shapes]]
        color = _matrices(plan, 1100 + c)
        _run(enc, afiles, amodel, layout, [P90], plan, "uint8", c == 3, alpha=alpha, color=color)
        post = [[{"blur": (1, 0.8)}, {"blur": (1, 2.0)}, {}, {"blur": (1, 0.5)}, {}, {"blur": (1, 1.0)}, {"blur": (1, 0.8)}]]
        _run(enc, afiles, amodel, layout, [P90S], plan, ("float16", "uint8")[c - 3], c == 4, consts=CONSTS[1], alpha=alpha, post=post)
        _run(enc, afiles, amodel, layout, [P90], plan, "uint8", False, alpha=alpha, color=color, post=post)


# ---- 5. NEAREST beside PREMULTIPLIED ----
@pytest.mark.parametrize("layout", LAYOUTS)
def test_nearest_beside_premultiplied_in_one_file(enc, afiles, amodel, layout):  # noqa: F811
    """one file with NEAREST views without an op and Lanczos PREMULTIPLIED views (the pair on ONE view is refused on the host): the
    launch runs the alpha instantiation over index tables too.  Both kinds of view equal the model, and the NEAREST views hold the
    file's own pixels only"""
    _check_conditions(afiles, [(i, WHOLE90, full) for i in (P90, P90S) for full in (UP90, DOWN90)], "lanczos")
    kinds = _kinds(layout)
    shapes = [(UP90, W130, "nearest", NONE), (UP90, W130, "lanczos", PRE), (DOWN90, None, "nearest", NONE), (DOWN90, D65, "lanczos", PRE), (UP90, W65, "nearest", TEAL)]
    own = {tuple(p) for p in afiles.planes[P90].reshape(4, -1).T.tolist()}
    for c in (3, 4):
        plan = [(c, [(WHOLE90, full, w, f, bool((k + c) & 1), kinds[(k + c) % len(kinds)]) for k, (full, w, f, _) in enumerate(shapes)]) for _ in (0, 1)]
        alpha = [[s[3] for s in shapes]] * 2
        _run(enc, afiles, amodel, layout, [P90, P90S], plan, ("uint8", "float32")[c - 3], c == 4, alpha=alpha)
    for full, w, f, a in shapes:
        pixels = {tuple(p) for p in amodel.view(P90, WHOLE90, full, w, f, a).reshape(4, -1).T.tolist()}
        assert (pixels <= own) == (f == "nearest" and a == NONE), (full, w, f)
