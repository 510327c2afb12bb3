"""GPU decoder of SEVERAL resized views of each file from one decode of it (-m gpu; fpng_amd_decode_batch_planar_views /
fpng_amd_decode_batch_device_planar_views: the crop kernels decode the bounding rectangle of the views' source boxes into the decode
scratch once, then dec_resize_exact_kernel writes every view from its own sub-rectangle of those planes, on a grid of exactly the
views' tiles): uint8 planes and the three float dtypes, three and four planes, both filters, mirrors, every pitch kind, host and
device files, one and several groups of files.

Expected values never come from the library: the pixels are the REFERENCE's decoder's (judge()), sliced to each view's crop,
resized WHOLE and sliced to the window by resize_view_model.py, and for the float dtypes looked up in test_gpu_decode_float's table:
what the view call must write for that view alone.  Buffers are sentinel-filled and compared WHOLE and bit for bit.

The shapes are the smallest at which the new code can go wrong: all ten views of a 600 x 130 file at once (boxes that start left of,
above, inside and past one another in shared planes; 1 x 1 windows beside 224 x 224 ones in one grid), a bounding rectangle that
starts past the first tile of the pixel pass, counts and plane counts that change from file to file (the prefix sum's boundaries),
and a host batch of more than one group (a group's range of records)."""
import numpy as np
import pytest

from test_gpu_decode import UNDECIDED, _device_files
from test_gpu_decode_float import CONSTS
from test_gpu_decode_layouts import SENTINEL, _damaged_files, _encode_gpu, _header_dims
from test_gpu_decode_planar import KINDS, _Region
from test_gpu_decode_resize import BITS, CROP_OUTSIDE, DTYPES, ELEM, _elements, _expect, _Files, _first_difference, enc, files  # noqa: F401  (enc, files: fixtures)
from test_gpu_resize_view import _cases, _Model, _window, model  # noqa: F401  (model: a fixture)
import resize_view_model as VM

pytestmark = pytest.mark.gpu


def _all_views(files, i, filter, k0=0):  # noqa: F811
    """every view of file i's size as (crop, full, window, filter, mirror, pitch kind): `filter` where the view runs with it, mirror
    flags alternating, pitch kinds dealt"""
    return [(crop, full, window, filter if filter in fs else fs[0], bool((k0 + k) & 1), KINDS[(k0 + k) % len(KINDS)])
            for k, (crop, full, window, fs) in enumerate(VM.VIEWS[files.dims[i]])]


def _decode(enc, pngs, plan, dtype, device, dev=None, consts=CONSTS[0]):  # noqa: F811
    """plan: per file (c, [(crop, full, window, filter, mirror, kind)]).  ONE call into ONE sentinel-filled buffer: (results, the
    elements' bits afterwards, the tensors per file, the regions in the records' order, the buffer's elements)"""
    import torch
    regs, off = [], 0
    for c, views in plan:
        for _, full, window, _, _, kind in views:
            r = _Region(off, *_window(full, window)[2:], c, kind)
            regs.append(r)
            off += r.size
    e = ELEM[dtype]
    buf = torch.full((off * e,), SENTINEL, dtype=torch.uint8, device="cuda")
    typed = buf.view(getattr(torch, dtype))
    it = iter(regs)
    per = [[next(it) for _ in views] for _, views in plan]
    outs = [[typed.as_strided((r.c, r.h, r.w), (r.pp, r.rp, 1), r.lo) for r in rs] for rs in per]
    kw = {} if dtype == "uint8" else {"scale": consts[0], "bias": consts[1]}
    args = ([[v[0] for v in views] for _, views in plan], outs, [[v[1] for v in views] for _, views in plan], [[v[2] for v in views] for _, views in plan],
            [[v[3] for v in views] for _, views in plan])
    kw.update(mirror=[[v[4] for v in views] for _, views in plan], order=[[r.order() for r in rs] for rs in per], bottom_up=[[r.kind == "bottom_up" for r in rs] for rs in per])
    if device:
        got = enc.decode_device_views(dev if dev is not None else _device_files(pngs, shift=1), *args, **kw)
    else:
        got = enc.decode_batch_views(pngs, *args, **kw)
    torch.cuda.synchronize()
    return got, buf.cpu().numpy().view(BITS[e]), outs, regs, off


def _sources(model, idx, plan, dtype, skip=()):  # noqa: F811
    """the (oh, ow, c) elements of every view, in the records' order (None for the views of the files in `skip`)"""
    return [None if n in skip else _elements(model.view(idx[n], crop, full, window, f), c, dtype, m)
            for n, (c, views) in enumerate(plan) for crop, full, window, f, m, _ in views]


def _run(enc, files, model, idx, plan, dtype, device, **kw):  # noqa: F811
    got, host, outs, regs, total = _decode(enc, [files.pngs[i] for i in idx], plan, dtype, device, **kw)
    assert len(got) == len(idx)
    for n, (i, (st, views, cf)) in enumerate(zip(idx, got)):
        assert st == 0 and cf == files.chans[i] and len(views) == len(outs[n]) and all(a is b for a, b in zip(views, outs[n])), (n, i, st, cf)
    exp = _expect(total, dtype, regs, _sources(model, idx, plan, dtype))
    diff = _first_difference(host, exp, regs)
    assert diff is None, (dtype, device, diff)


@pytest.mark.parametrize("filter", VM.FILTERS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", [3, 4])
def test_all_views_of_a_size_at_once_device_files(enc, files, model, c, dtype, filter):  # noqa: F811
    """every file with ALL the views of its size as views of that one file -- ten for a 600 x 130 file -- in ONE call into ONE
    buffer that is compared whole"""
    idx = list(range(len(files.pngs)))
    assert sum(d == (600, 130) for d in files.dims) == 6 and len(VM.VIEWS[(600, 130)]) == 10
    _run(enc, files, model, idx, [(c, _all_views(files, i, filter, k0=i + c)) for i in idx], dtype, True)


@pytest.mark.parametrize("c,dtype,filter", [(3, "uint8", "bicubic"), (4, "bfloat16", "bilinear"), (4, "float32", "bicubic")])
def test_all_views_of_a_size_at_once_host_files(enc, files, model, c, dtype, filter):  # noqa: F811
    """the same through fpng_amd_decode_batch_planar_views (files in host memory), for a subset"""
    idx = list(range(len(files.pngs)))[::2]
    _run(enc, files, model, idx, [(c, _all_views(files, i, filter, k0=2 * i + c)) for i in idx], dtype, False)


@pytest.mark.parametrize("filter", VM.FILTERS)
@pytest.mark.parametrize("dtype", ["uint8", "float16"])
def test_a_bounding_box_that_starts_past_the_first_tile(enc, files, model, dtype, filter):  # noqa: F811
    """two views of each 600 x 130 file whose boxes both lie past the first 256-column block and the first 48-row segment and do
    not touch: the planes in the scratch are the bounding rectangle's, and each view is addressed relative to it, not to its crop"""
    import fpng_amd
    crop, full, wins = (0, 0, 600, 130), (300, 65), [(140, 30, 20, 10), (235, 48, 65, 17)]
    box = fpng_amd.views_source([crop, crop], full, wins, filter)
    assert box[0] > 256 and box[1] > 48 and fpng_amd.crop_tiles(600, 130, box)[1] == 1
    idx = [i for i, d in enumerate(files.dims) if d == (600, 130)]
    for order in (wins, wins[::-1]):  # (the box that starts first as the file's second record too)
        plan = [(3 + (n & 1), [(crop, full, w, filter, bool(k & 1), KINDS[(n + k) % len(KINDS)]) for k, w in enumerate(order)]) for n in range(len(idx))]
        _run(enc, files, model, idx, plan, dtype, True)


def _mixed_counts(files, k0):  # noqa: F811
    """counts 1, 10, 2, 1 over a stored 4-channel, a 2-pass 4-channel, a stored 3-channel and a 1-pass 3-channel file, into 4, 3, 4
    and 3 planes: planes and tile counts change from record to record"""
    idx = [13, 4, 2, 6]
    assert [files.dims[i] for i in idx] == [(64, 97), (600, 130), (600, 130), (257, 49)] and [files.chans[i] for i in idx] == [4, 4, 3, 3]
    assert [len(files.pngs[i]) > files.dims[i][0] * files.dims[i][1] * files.chans[i] for i in idx] == [True, False, True, False]  # (stored: longer than its pixels)
    views = [_all_views(files, 13, "bicubic", k0), _all_views(files, 4, "bicubic", k0 + 1), _all_views(files, 2, "bilinear", k0 + 2)[1:3], _all_views(files, 6, "bilinear", k0 + 4)]
    assert [len(v) for v in views] == [1, 10, 2, 1]
    return idx, [(c, v) for c, v in zip((4, 3, 4, 3), views)]


@pytest.mark.parametrize("device", [False, True])
def test_mixed_counts_in_one_batch(enc, files, model, device):  # noqa: F811
    """counts 1, 10, 2, 1 in one call, f16, every pitch kind dealt across the views, both filters and mirrors in one file"""
    for k0 in (0, 3):
        idx, plan = _mixed_counts(files, k0)
        assert {v[5] for _, views in plan for v in views} == set(KINDS)
        _run(enc, files, model, idx, plan, "float16", device)


@pytest.fixture(scope="module")
def big_files(enc):  # noqa: F811
    """three stored 1024 x 1024 RGBA `noise` files: 12 MiB of stream, so a host batch of them forms more than one group"""
    import fpng_amd
    items = [(fpng_amd.synth_image("noise", 1024, 1024, 4, seed=70 + k), 2) for k in range(3)]
    pngs = [bytes(p) for p in _encode_gpu(enc, items)]
    assert all(len(p) > 4 << 20 for p in pngs)  # (decode_api.cpp's rule: host files, >= 8 MiB of stream, more than one file)
    return _Files(pngs, [(1024, 1024)] * 3, [4] * 3)


@pytest.mark.parametrize("dtype", ["uint8", "bfloat16"])
def test_more_than_one_group(enc, big_files, dtype):  # noqa: F811
    """2, 1 and 3 small views of three large host files: every group launches its own jobs' range of the records"""
    plan = [(3, [((1000, 1000, 24, 24), (12, 12), None, "bilinear", False, "packed"), ((3, 5, 40, 30), (20, 15), (2, 2, 8, 8), "bicubic", True, "odd")]),
            (4, [((500, 700, 64, 16), (8, 2), None, "bicubic", True, "reversed")]),
            (3, [((0, 0, 9, 9), (27, 27), (20, 20, 7, 7), "bicubic", False, "bottom_up"), ((1015, 0, 9, 1024), (3, 32), None, "bilinear", True, "pad256"),
                 ((512, 512, 16, 16), (16, 16), (0, 0, 16, 1), "bilinear", False, "packed")])]
    _run(enc, big_files, _Model(big_files), [0, 1, 2], plan, dtype, False)


@pytest.mark.parametrize("c,dtype,filter,device", [(3, "uint8", "bilinear", True), (4, "float16", "bicubic", True), (3, "float32", "bicubic", False)])
def test_one_view_per_file_is_the_view_call(enc, files, model, c, dtype, filter, device):  # noqa: F811
    """view_count = 1 everywhere, over the view call's own cases: the buffer the model gives for that call"""
    cases = _cases(files, filter)
    plan = [(c, [(crop, full, window, filter, bool(k & 1), KINDS[(k + c) % len(KINDS)])]) for k, (_, crop, full, window) in enumerate(cases)]
    _run(enc, files, model, [k[0] for k in cases], plan, dtype, device)


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("dtype", ["uint8", "float16"])
def test_statuses(enc, files, model, dtype, device):  # noqa: F811
    """One of a file's three views has a crop that leaves the image: the FILE gets status 67 and none of its regions is touched.  A
    damaged file gets the status the CROP call gives it for views_source()'s box, and nothing outside its views' spans is written.
    Every other file is exact."""
    import fpng_amd
    damaged = None
    for p in _damaged_files():
        w, h = _header_dims(p)
        if not (2 <= w <= 600 and 2 <= h <= 600):
            continue
        dviews = [((0, h - 2, w, 2), (max(w // 3, 1), 3), None, "bicubic", True, "odd"), ((0, 0, min(w, 5), 1), (3, 3), (1, 1, 2, 2), "bilinear", False, "packed")]
        box = fpng_amd.views_source([v[0] for v in dviews], [v[1] for v in dviews], [v[2] for v in dviews], [v[3] for v in dviews])
        (st, _, _), = enc.decode_batch_crop([p], [box])
        if st not in (0, UNDECIDED):
            damaged = (p, dviews, st)
            break
    assert damaged is not None
    idx, plan = _mixed_counts(files, 1)
    outside = [plan[2][1][0], ((files.dims[2][0] - 1, 0, 2, 1), (7, 5), (1, 1, 5, 3), "bicubic", False, "pad256"), plan[2][1][1]]
    plan[2] = (plan[2][0], outside)
    plan.append((3, damaged[1]))
    pngs = [files.pngs[i] for i in idx] + [damaged[0]]
    got, host, outs, regs, total = _decode(enc, pngs, plan, dtype, device)
    assert [st for st, _, _ in got] == [0, 0, CROP_OUTSIDE, 0, damaged[2]] and got[2][1] is None
    assert (got[2][2], got[4][1]) == (files.chans[idx[2]], None)
    exp = _expect(total, dtype, regs, _sources(model, idx + [None], plan, dtype, skip=(2, 4)))
    for r in regs[-2:]:  # (what a rejected file's spans hold is not defined)
        for a, b in r.spans():
            exp[a:b] = host[a:b]
    assert _first_difference(host, exp, regs) is None, _first_difference(host, exp, regs)


@pytest.mark.parametrize("device", [False, True])
def test_checksums_verified(enc, files, model, device):  # noqa: F811
    """set_decode_verify(CRC-32 and Adler-32): every tile of every file runs under the Adler-32 check while the crop stage still
    writes the bounding box; the outputs are the same and the statuses are the crop call's under the same flags"""
    import fpng_amd
    idx, plan = _mixed_counts(files, 2)
    pngs = [files.pngs[i] for i in idx]
    boxes = [fpng_amd.views_source([v[0] for v in views], [v[1] for v in views], [v[2] for v in views], [v[3] for v in views]) for _, views in plan]
    try:
        enc.set_decode_verify(fpng_amd.VERIFY_CRC32 | fpng_amd.VERIFY_ADLER32)
        want = [st for st, _, _ in (enc.decode_device_crop(_device_files(pngs), boxes) if device else enc.decode_batch_crop(pngs, boxes))]
        assert want == [0] * len(idx)
        _run(enc, files, model, idx, plan, "bfloat16", device)
    finally:
        enc.set_decode_verify(0)


def test_a_descriptor_decodes_again_after_its_outputs_are_overwritten(enc, files, model):  # noqa: F811
    import torch
    idx, plan = _mixed_counts(files, 0)
    dev = _device_files([files.pngs[i] for i in idx], shift=2)
    for dtype in ("uint8", "float32"):
        outs = [[torch.zeros((c,) + _window(full, window)[:1:-1], dtype=getattr(torch, dtype), device="cuda") for _, full, window, *_ in views] for c, views in plan]
        kw = {} if dtype == "uint8" else {"scale": CONSTS[0][0], "bias": CONSTS[0][1]}
        nest = [[[v[k] for v in views] for _, views in plan] for k in range(5)]
        db = enc.make_decode_batch_views(dev, nest[0], outs, nest[1], nest[2], nest[3], mirror=nest[4], **kw)
        want = _sources(model, idx, plan, dtype)
        for again in range(2):
            for ts in outs:
                for t in ts:
                    t.fill_(1)
            assert enc.decode_device_views(db, results=False) is db
            torch.cuda.synchronize()
            assert list(db.statuses()) == [0] * len(idx)
            for k, t in enumerate(t for ts in outs for t in ts):
                bits = t.cpu().view(torch.uint8).numpy().view(BITS[ELEM[dtype]])
                assert np.array_equal(bits, want[k].transpose(2, 0, 1)), (dtype, again, k)
    with pytest.raises(ValueError):
        enc.decode_device_resize_view(db)  # (another call's descriptor)
    with pytest.raises(ValueError):
        enc.decode_batch_views(db)  # (device files: decode_device_views)
    got = enc.decode_device_views(dev[:2], [[(0, 0, 64, 97)], [(0, 0, 600, 130)] * 2], full=(96, 96), dtype=torch.float16)  # (outs=None allocates)
    assert [len(ts) for _, ts, _ in got] == [1, 2] and all(st == 0 and t.dtype == torch.float16 and tuple(t.shape) == (3, 96, 96) for st, ts, _ in got for t in ts)
