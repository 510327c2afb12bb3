"""The five resize kernels where their tests had not been (-m gpu): FULL 64 x 16 tiles at and just under the scale limits, a
rectangular launch that is split, and an exact grid over a thousand records.

Full tiles (resize_limit_views.LIMIT_VIEWS, of two 2080 x 768 files -- stored 3-channel `noise`, compressed 4-channel `blocks`): at
32 x (bilinear) / 16 x (bicubic) a tile's 16 output rows reach 544 / 304 source rows, the T buffer comes within three rows of
r.rows (547 / 307), the launch's dynamic LDS is the documented 56 448 / 41 088 bytes, and the horizontal pass runs 64 taps across a
full 64-lane tile row.  Every kernel has `nrows = min(.., r.rows)`: were the host's bound short, rows would be dropped silently, and
a launch refused for its LDS would leave the sentinel -- both with status 0, so only the bytes can tell.  Through dec_resize_kernel
(the plain resize call and the view call), dec_resize_exact_kernel, dec_resize_hwc_kernel and dec_resize_color_kernel (planar and
channels-last), uint8 / float16 (the dword stores) / float32 (channels-last), 3 and 4 channels, mirror off and on, device and host files.

Expected bytes never come from the library: the reference decoder's planes (judge()), resized WHOLE by resize_view_model
(test_resize_bounds_cpu.py pins it to Pillow at exactly these scales), sliced to the window, through test_gpu_decode_float's table
or color_model.  Sentinel-filled buffers are compared WHOLE and bit for bit; every status is 0; every view is shown to be inside the
limits (fpng_amd.resize_view_source answers, and answers the model's box) before the call, so a refusal cannot pass for a test.

That these comparisons see the faults they are here for was shown on the host, with expected buffers from deliberately wrong
models: a tile model whose T buffer is one row shorter than its 16 rows reach, and a batch model without the records behind the
first launch, each differ from the right model's buffer in the very views below (test_resize_bounds_cpu.py's last test, and the
last one here)."""
import time

import numpy as np
import pytest

from test_gpu_decode import _device_files
from test_gpu_decode_float import CONSTS, _bits as _table_bits, _tables
from test_gpu_decode_layouts import _encode_gpu
from test_gpu_decode_planar import KINDS as PLANAR_KINDS
from test_gpu_decode_resize import _decode_resize, _elements, _expect, _Files, _first_difference, _regions, enc, files  # noqa: F401  (enc, files: fixtures)
from test_gpu_decode_views_color import _decode as _decode_views, _difference, _matrices, _sources as _color_sources
from test_gpu_resize_view import _decode_view, _Model, _window, model  # noqa: F401  (model: a fixture)
import resize_limit_views as LV
import resize_view_model as VM

pytestmark = pytest.mark.gpu

HWC_KINDS = ["tight", "odd", "px4", "reversed", "bottom_up"]
KINDS = {"planar": PLANAR_KINDS, "hwc": HWC_KINDS}


def _matrix(dtypes):
    """(c, dtype, mirror, device files): every combination on device files, and one with the files in host memory"""
    return [(c, d, m, True) for c in (3, 4) for d in dtypes for m in (False, True)] + [(3, dtypes[-1], True, False)]


@pytest.fixture(scope="module")
def limit_files(enc):  # noqa: F811
    import fpng_amd
    w, h = LV.LIMIT_FILE
    items = [(fpng_amd.synth_image("noise", w, h, 3, seed=501), 2), (fpng_amd.synth_image("blocks", w, h, 4, seed=502), 0)]
    pngs = [bytes(p) for p in _encode_gpu(enc, items)]
    assert len(pngs[0]) > w * h * 3 and len(pngs[1]) < w * h * 4  # (stored: longer than its pixels; compressed)
    return _Files(pngs, [LV.LIMIT_FILE] * 2, [3, 4])


@pytest.fixture(scope="module")
def limit_model(limit_files):
    return _Model(limit_files)


def _accepted(views):
    """every (crop, full, window, filter) is inside the documented limits, and the library says so"""
    import fpng_amd
    for crop, full, window, f in views:
        assert crop[2] <= VM.MAX_SCALE[f] * full[0] and crop[3] <= VM.MAX_SCALE[f] * full[1], (crop, full, f)
        assert fpng_amd.resize_view_source(crop, full, window, f) == VM.view_source(crop, full, window, f), (crop, full, window, f)  # (a refusal raises)


def _plan(views_per_file, c, layout, mirror=None):
    """per file (c, [(crop, full, window, filter, mirror, kind)]): destination kinds dealt across the views; c: one for all files, or
    one per file; mirror None: flags alternating"""
    kinds, k, plan = KINDS[layout], 0, []
    for n, views in enumerate(views_per_file):
        cn = c if isinstance(c, int) else c[n]
        plan.append((cn, [(crop, full, window, f, bool((k + j) & 1) if mirror is None else mirror, kinds[(k + j + cn) % len(kinds)]) for j, (crop, full, window, f) in enumerate(views)]))
        k += len(views)
    return plan


_TABLES = {}


def _view_sources(mdl, idx, plan, dtype):
    """test_gpu_decode_views' _sources -- the (oh, ow, c) elements of every view in the records' order, the model's bytes through
    test_gpu_decode_float's table -- with the table made once per dtype, not once per view: a plan here has 1200 of them"""
    if dtype != "uint8" and dtype not in _TABLES:
        _TABLES[dtype] = _tables(CONSTS[0], dtype)
    out = []
    for n, (c, views) in enumerate(plan):
        for crop, full, window, f, m, _ in views:
            r4 = mdl.view(idx[n], crop, full, window, f)
            px = np.ascontiguousarray((r4[:c, :, ::-1] if m else r4[:c]).transpose(1, 2, 0))
            out.append(px if dtype == "uint8" else _table_bits(px, _TABLES[dtype]))
    return out


def _run_views(enc, fs, mdl, layout, idx, plan, dtype, device, color, dev=None):  # noqa: F811
    """the planar or channels-last views call, plain (color None) or with a matrix per view, against the model: whole buffer, all statuses 0"""
    _accepted([v[:4] for _, views in plan for v in views])
    t0 = time.perf_counter()
    got, host, outs, regs = _decode_views(enc, layout, [fs.pngs[i] for i in idx], plan, dtype, device, color, dev=dev)
    took = time.perf_counter() - t0
    assert len(got) == len(idx)
    for n, (i, (st, views, cf)) in enumerate(zip(idx, got)):
        assert st == 0 and cf == fs.chans[i] and len(views) == len(outs[n]), (n, i, st, cf)
    sources = _view_sources(mdl, idx, plan, dtype) if color is None else _color_sources(mdl, idx, plan, dtype, color)
    diff = _difference(layout, host, dtype, regs, sources)
    assert diff is None, (layout, dtype, device, diff)
    return took


# ---- full tiles at and just under the scale limits ----
@pytest.mark.parametrize("c,dtype,mirror,device", _matrix(["uint8", "float16"]))
def test_full_tiles_plain_resize_call(enc, limit_files, limit_model, c, dtype, mirror, device):  # noqa: F811
    """dec_resize_kernel<.., false> on the rectangular grid: the bilinear views without a window, of both files"""
    views = [v for v in LV.LIMIT_VIEWS if v[2] is None and v[3] == "bilinear"]
    assert len(views) == 5
    _accepted(views)
    cases = [(i, crop, full) for i in (0, 1) for crop, full, _, _ in views]
    kinds = [PLANAR_KINDS[(k + c) % len(PLANAR_KINDS)] for k in range(len(cases))]
    regs, total = _regions([full for _, _, full in cases], c, kinds)
    got, host, outs = _decode_resize(enc, [limit_files.pngs[i] for i, _, _ in cases], [crop for _, crop, _ in cases], regs, total, dtype, device, [mirror] * len(cases))
    assert [(st, cf) for st, _, cf in got] == [(0, limit_files.chans[i]) for i, _, _ in cases]
    exp = _expect(total, dtype, regs, [_elements(limit_model.view(i, crop, full, None, "bilinear"), c, dtype, mirror) for i, crop, full in cases])
    diff = _first_difference(host, exp, regs)
    assert diff is None, (c, dtype, device, diff, [cases[j] for j, *_ in diff[4]])


@pytest.mark.parametrize("c,dtype,mirror,device", _matrix(["uint8", "float16"]))
def test_full_tiles_view_call(enc, limit_files, limit_model, c, dtype, mirror, device):  # noqa: F811
    """dec_resize_kernel<.., true>: every view of both files, windows and both filters, in one launch whose LDS is the bilinear limit's"""
    _accepted(LV.LIMIT_VIEWS)
    cases = [(i,) + v for i in (0, 1) for v in LV.LIMIT_VIEWS]
    kinds = [PLANAR_KINDS[(k + c) % len(PLANAR_KINDS)] for k in range(len(cases))]
    regs, total = _regions([_window(full, window)[2:] for _, _, full, window, _ in cases], c, kinds)
    got, host, outs = _decode_view(enc, [limit_files.pngs[k[0]] for k in cases], [k[1] for k in cases], [k[2] for k in cases], [k[3] for k in cases], [k[4] for k in cases], regs, total,
                                   dtype, device, [mirror] * len(cases))
    assert [(st, cf) for st, _, cf in got] == [(0, limit_files.chans[k[0]]) for k in cases]
    exp = _expect(total, dtype, regs, [_elements(limit_model.view(*case), c, dtype, mirror) for case in cases])
    diff = _first_difference(host, exp, regs)
    assert diff is None, (c, dtype, device, diff, [cases[j] for j, *_ in diff[4]])


def test_the_first_view_is_the_plain_resize_call(enc, limit_files):  # noqa: F811
    """2080 x 768 -> 65 x 24, no window, bilinear: the view call writes byte for byte what decode_device_resize writes, mirrored or
    not, bytes and f16 (test_gpu_resize_view's equality, at 32 x)"""
    import torch
    crop, full, window, f = LV.LIMIT_VIEWS[0]
    assert window is None and f == "bilinear"
    dev = _device_files(limit_files.pngs)
    for dtype, kw in ((torch.uint8, {}), (torch.float16, {"mean": (0.485, 0.456, 0.406), "std": (0.229, 0.224, 0.225)})):
        a = torch.full((2, 3, full[1], full[0]), 7, dtype=dtype, device="cuda")
        b = torch.full((2, 3, full[1], full[0]), 9, dtype=dtype, device="cuda")
        got_a = enc.decode_device_resize(dev, [crop] * 2, list(a), mirror=[False, True], **kw)
        got_b = enc.decode_device_resize_view(dev, [crop] * 2, list(b), full, mirror=[False, True], **kw)
        torch.cuda.synchronize()
        assert [st for st, _, _ in got_a] == [st for st, _, _ in got_b] == [0, 0]
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)) and not bool((a == 7).all()), dtype


@pytest.mark.parametrize("c,dtype,mirror,device", _matrix(["uint8", "float16"]))
def test_full_tiles_planar_views_call(enc, limit_files, limit_model, c, dtype, mirror, device):  # noqa: F811
    """dec_resize_exact_kernel: all of a file's views as views of that one file"""
    _run_views(enc, limit_files, limit_model, "planar", [0, 1], _plan([LV.LIMIT_VIEWS] * 2, c, "planar", mirror), dtype, device, None)


@pytest.mark.parametrize("c,dtype,mirror,device", _matrix(["uint8", "float16", "float32"]))
def test_full_tiles_channels_last_views_call(enc, limit_files, limit_model, c, dtype, mirror, device):  # noqa: F811
    """dec_resize_hwc_kernel: the same plan into tight, odd-pitched, 4-element, reversed and bottom-up channels-last destinations"""
    plan = _plan([LV.LIMIT_VIEWS] * 2, c, "hwc", mirror)
    assert {v[5] for _, views in plan for v in views} == set(HWC_KINDS)
    _run_views(enc, limit_files, limit_model, "hwc", [0, 1], plan, dtype, device, None)


@pytest.mark.parametrize("c,dtype,mirror,device", _matrix(["uint8", "float16"]))
def test_full_tiles_planar_colour_call(enc, limit_files, limit_model, c, dtype, mirror, device):  # noqa: F811
    """dec_resize_color_kernel<.., false>: the same plan, a different matrix for every view"""
    plan = _plan([LV.LIMIT_VIEWS] * 2, c, "planar", mirror)
    _run_views(enc, limit_files, limit_model, "planar", [0, 1], plan, dtype, device, _matrices(plan, 2080 + c))


@pytest.mark.parametrize("c,dtype,mirror,device", _matrix(["uint8", "float16", "float32"]))
def test_full_tiles_channels_last_colour_call(enc, limit_files, limit_model, c, dtype, mirror, device):  # noqa: F811
    """dec_resize_color_kernel<.., true>: the waves' row buffers take the place of weights laid out for 65 taps and 547 rows"""
    plan = _plan([LV.LIMIT_VIEWS] * 2, c, "hwc", mirror)
    _run_views(enc, limit_files, limit_model, "hwc", [0, 1], plan, dtype, device, _matrices(plan, 768 + c))


# ---- a batch of 600 files ----
class _Batch:
    """600 files: four tiny ones (64 x 97 and 1 x 1, three and four channels) taking turns, and a stored 3-channel 600 x 130 `noise`
    file at index 590; in device memory once"""

    def __init__(self, files):  # noqa: F811
        self.tiny = [i for i, d in enumerate(files.dims) if d in ((64, 97), (1, 1))]
        self.big = [i for i, d in enumerate(files.dims) if d == (600, 130) and files.chans[i] == 3][2]
        assert len(self.tiny) == 4 and len(files.pngs[self.big]) > 600 * 130 * 3  # (stored)
        self.idx = [self.big if k == LV.SPLIT_AT else self.tiny[k % 4] for k in range(LV.SPLIT_FILES)]
        self.dev = _device_files([files.pngs[i] for i in self.idx], shift=1)


@pytest.fixture(scope="module")
def batch(files):  # noqa: F811
    return _Batch(files)


@pytest.fixture(scope="module")
def split_planes(files, batch):  # noqa: F811
    """the model's three planes of the large record, 600 x 130 -> 4096 x 1792: computed once, read-only"""
    r = VM.view_planes(files.planes[batch.big][:3], LV.SPLIT_SIZE, None, "bilinear")
    r.setflags(write=False)
    return r


def _split_records(files, batch):  # noqa: F811
    """(file, crop, size, filter, mirror, kind) of the 600 records: outputs 1 x 1 .. 5 x 5, and 4096 x 1792 at index 590"""
    recs = []
    for k, i in enumerate(batch.idx):
        if k == LV.SPLIT_AT:
            recs.append((i, LV.SPLIT_CROP, LV.SPLIT_SIZE, "bilinear", True, "packed"))
        else:
            crop, size = LV.tiny_view(k, files.dims[i])
            recs.append((i, crop, size, "bilinear", bool(k & 1), PLANAR_KINDS[k % len(PLANAR_KINDS)]))
    return recs


def _split_expected(files, model, split_planes, recs, total, regs, last=None):  # noqa: F811
    """the buffer the model gives for records 0 .. last - 1 (None: all of them)"""
    src = [None if last is not None and k >= last else
           _elements(split_planes if size == LV.SPLIT_SIZE else model.view(i, crop, size, None, f), 3, "uint8", m) for k, (i, crop, size, f, m, _) in enumerate(recs)]
    return _expect(total, "uint8", regs, src)


@pytest.mark.parametrize("call", ["resize", "view"])
def test_a_rectangular_launch_that_is_split(enc, files, model, batch, split_planes, call):  # noqa: F811
    """launch_dec_resize cuts a batch into launches of step = min(32768, (2^32 - 1) / (max_tiles * 4 * 256)) records.  The record
    at index 590 has 64 x 112 = 7168 tiles, so step = 585 < 600: the first launch is a grid of (7168, 4, 585) workgroups sized by a
    record it does not hold -- 16.8 million workgroups, all but ~1800 of which leave at once -- and the second launch starts at
    recs + 585 and holds the large record.  A wrong step or offset skips or repeats whole files with status 0.  Files in device
    memory are ONE group whatever their size (plan_groups: only host files of 8 MiB and more are cut into groups), so the group's
    one call to launch_dec_resize holds all 600 records.

    Observed on an MI355X: the call with its synchronisation takes 0.009 s (plain resize call) and 0.008 s (view call), the 21 MiB
    copy back included; the case cannot be made smaller, since the step always fills the budget of 2^32 threads."""
    recs = _split_records(files, batch)
    n, tiles = len(recs), max(((w + 63) // 64) * ((h + 15) // 16) for _, _, (w, h), *_ in recs)
    step = LV.split_step(tiles)
    assert tiles == 7168 and step == 585 and n > step > 0 and step <= LV.SPLIT_AT < n
    _accepted([(crop, size, None, f) for _, crop, size, f, _, _ in recs])
    regs, total = _regions([size for _, _, size, *_ in recs], 3, [r[5] for r in recs])
    t0 = time.perf_counter()
    if call == "resize":
        got, host, _ = _decode_resize(enc, None, [r[1] for r in recs], regs, total, "uint8", True, [r[4] for r in recs], dev=batch.dev)
    else:
        got, host, _ = _decode_view(enc, None, [r[1] for r in recs], [r[2] for r in recs], [None] * n, [r[3] for r in recs], regs, total, "uint8", True, [r[4] for r in recs],
                                    dev=batch.dev)
    print("split launch, %s call: %.3f s with its synchronisation and the copy back" % (call, time.perf_counter() - t0))
    assert [(st, cf) for st, _, cf in got] == [(0, files.chans[r[0]]) for r in recs]
    diff = _first_difference(host, _split_expected(files, model, split_planes, recs, total, regs), regs)
    assert diff is None, (call, diff)


@pytest.mark.parametrize("color", [False, True])
@pytest.mark.parametrize("layout", ["planar", "hwc"])
def test_an_exact_grid_over_a_thousand_records(enc, files, model, batch, layout, color):  # noqa: F811
    """the same 600 files with 1 + (k mod 3) tiny views each and a 129 x 33 window (nine tiles) in file 590's place of the large
    one: the binary search over pre[] of dec_resize_exact_kernel, dec_resize_hwc_kernel and dec_resize_color_kernel runs over
    1200 records instead of fourteen; both filters, mirrors, every destination kind, a different matrix per record, float16"""
    views_per_file = []
    for k, i in enumerate(batch.idx):
        if k == LV.SPLIT_AT:
            views = [(LV.SPLIT_CROP, LV.MANY_FULL, LV.MANY_WINDOW, "bicubic"), ((5, 7, 9, 11), (3, 3), None, "bilinear"), ((250, 40, 13, 20), (5, 5), None, "bicubic")]
        else:
            views = [LV.tiny_view(k + 7 * j, files.dims[i]) + (None, VM.FILTERS[(k + j) & 1]) for j in range(1 + k % 3)]
        assert len(views) == 1 + k % 3
        views_per_file.append(views)
    plan = _plan(views_per_file, [3 + (k & 1) for k in range(len(views_per_file))], layout)
    assert sum(len(v) for _, v in plan) == 1200 and {v[5] for _, views in plan for v in views} == set(KINDS[layout])
    _run_views(enc, files, model, layout, batch.idx, plan, "float16", True, _matrices(plan, 600) if color else None, dev=batch.dev)


# ---- the comparison above sees the fault it is here for (host arithmetic only: no kernel is run wrong) ----
def test_a_launch_that_skips_the_records_behind_the_first_would_be_seen(files, model, batch, split_planes):  # noqa: F811
    """the expected buffer of a model that stops at record `step` differs from the right one in every file behind it"""
    recs = _split_records(files, batch)
    regs, total = _regions([size for _, _, size, *_ in recs], 3, [r[5] for r in recs])
    step = LV.split_step(7168)
    right = _split_expected(files, model, split_planes, recs, total, regs)
    wrong = _split_expected(files, model, split_planes, recs, total, regs, last=step)
    diff = _first_difference(wrong, right, regs)
    differ = wrong != right
    assert diff is not None and diff[4][0][0] == step and {i for i, r in enumerate(regs) if differ[r.off:r.off + r.size].any()} == set(range(step, len(recs)))
