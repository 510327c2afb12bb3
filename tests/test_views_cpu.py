"""No-GPU tests of the VIEWS interface (fpng_amd_decode_batch(_device)_planar_views, fpng_amd_views_source: several resized views of
each file from one decode of it): the exported symbols and the fpng_amd_view_dest record, the box a file decodes against the
bounding rectangle of resize_view_model.view_source, every call-level refusal -- none of which needs an encoder or a device -- and
the descriptor make_decode_batch_views builds from CPU tensor views, with its nesting and broadcast rules."""
import ctypes as C
import itertools

import pytest
import torch

import fpng_amd
from fpng_amd import _lib
from fpng_amd.api import Encoder

import resize_view_model as VM
from test_resize_cpu import DTYPES
from test_resize_view_cpu import BAD, GOOD

NAMES = ("fpng_amd_decode_batch_planar_views", "fpng_amd_decode_batch_device_planar_views", "fpng_amd_views_source")


def test_entry_points_and_record(built_lib):
    lib = _lib.load()
    for name in NAMES:
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None
    assert lib.fpng_amd_abi_version() == 5  # (new entry points, the same ABI version)
    assert C.sizeof(_lib.ViewDest) == 32
    assert {n: getattr(_lib.ViewDest, n).offset for n, _ in _lib.ViewDest._fields_} == {"d_pixels": 0, "row_pitch": 8, "plane_pitch": 16, "pixels_cap": 24}
    assert C.sizeof(_lib.ResizeView) == 32 and C.sizeof(_lib.Crop) == 16 and C.sizeof(_lib.PngPlanarIn) == 48  # (the records around it are what they were)


def _bounding(boxes):
    x0, y0 = min(b[0] for b in boxes), min(b[1] for b in boxes)
    return x0, y0, max(b[0] + b[2] for b in boxes) - x0, max(b[1] + b[3] for b in boxes) - y0


def _flat():
    """(crop, full, window, filter) of every view of VIEWS[(600, 130)] in every filter it runs with"""
    return [(crop, full, window, f) for crop, full, window, fs in VM.VIEWS[(600, 130)] for f in fs]


def test_views_source_is_the_bounding_rectangle(built_lib):
    flat = _flat()
    assert len(flat) == 18
    sets = [flat] + [list(p) for p in itertools.combinations(flat, 2)] + [[v] for v in flat]
    bigger = 0
    for views in sets:
        crops, fulls, windows, filters = ([v[k] for v in views] for k in range(4))
        box = fpng_amd.views_source(crops, fulls, windows, filters)
        each = [VM.view_source(*v) for v in views]
        assert box == _bounding(each), views
        if len(views) == 1:
            assert box == fpng_amd.resize_view_source(*views[0])
        bigger += len(views) == 2 and box[2] * box[3] > sum(b[2] * b[3] for b in each)  # (two boxes apart: everything between them)
    assert bigger > 0
    # the two views of the GPU test "a bounding box that starts past the first tile": past the first 256-column block and the first
    # 48-row segment, not touching each other, and the bounding rectangle runs fewer tiles than the whole file
    crop, full = (0, 0, 600, 130), (300, 65)
    for f in VM.FILTERS:
        a, b = VM.view_source(crop, full, (140, 30, 20, 10), f), VM.view_source(crop, full, (235, 48, 65, 17), f)
        assert a[0] > 256 and a[1] > 48 and b[0] >= a[0] + a[2] and b[1] >= a[1] + a[3]
        box = fpng_amd.views_source([crop, crop], full, [(140, 30, 20, 10), (235, 48, 65, 17)], f)  # (full and filter: one for all)
        assert box == _bounding([a, b]) and box[0] > 256 and box[1] > 48
        nseg, first, ncb = fpng_amd.crop_tiles(600, 130, box)
        whole = fpng_amd.crop_tiles(600, 130, crop)
        assert first == 1 and nseg * ncb < whole[0] * whole[2]
    # views whose crops differ: the rectangle is in the FILE's coordinates
    assert fpng_amd.views_source([(5, 7, 9, 11), (250, 40, 13, 20)], [(65, 17), (13, 20)]) == (5, 7, 258, 53)
    with pytest.raises(ValueError):
        fpng_amd.views_source([(-1, 0, 5, 5)], (5, 5))
    with pytest.raises(ValueError):
        fpng_amd.views_source([crop, crop], [full])  # (one per view, or one for all)
    with pytest.raises(fpng_amd.FpngAmdError):
        fpng_amd.views_source([], (5, 5))


def _arrays(records, counts):
    """(files, view_count, crops, views, dests, results) with empty destination fields in `files`"""
    total, n = len(records), len(counts)
    files, cnt = (_lib.PngPlanarIn * n)(), (C.c_uint32 * n)(*counts)
    c, v, d = (_lib.Crop * total)(), (_lib.ResizeView * total)(), (_lib.ViewDest * total)()
    for k, (crop, view) in enumerate(records):
        c[k].x, c[k].y, c[k].w, c[k].h = crop
        v[k].full_w, v[k].full_h, v[k].x, v[k].y, v[k].w, v[k].h, v[k].flags, v[k].filter = view
    for f in files:
        f.num_chans = 3
    return files, cnt, c, v, d, (_lib.DecodeResult * n)()


def test_call_level_refusals_need_no_encoder(built_lib):
    """Everything that needs no file is judged before the encoder is looked at: with a NULL encoder every call returns -1 and the
    message names the reason -- a bad argument its own, a good set only the missing encoder"""
    lib = _lib.load()
    fmt = _lib.FloatFormat()

    def why():
        return lib.fpng_amd_last_error().decode()

    for fn in (lib.fpng_amd_decode_batch_planar_views, lib.fpng_amd_decode_batch_device_planar_views):
        files, cnt, c, v, d, res = _arrays([GOOD[0], GOOD[1], GOOD[2]], [2, 1])
        good = [files, 2, cnt, c, v, d, None, res]
        assert fn(None, *good) == -1 and "null/empty batch" in why(), why()  # (nothing is at fault -- the batch has no encoder)
        assert fn(None, files, 2, cnt, c, v, d, C.byref(fmt), res) == -1 and "null/empty batch" in why(), why()
        for k in (0, 2, 3, 4, 5, 7):  # a null array
            args = list(good)
            args[k] = None
            assert fn(None, *args) == -1 and "null files, view_count, crops, views, dests or results" in why(), (k, why())
        for counts in ([0, 3], [3, 0], [0, 0]):  # a view_count of 0
            assert fn(None, files, 2, (C.c_uint32 * 2)(*counts), c, v, d, None, res) == -1 and "view_count of 0" in why(), (counts, why())
        # a sum that does not fit 32 bits (refused before any record is read: the arrays hold three)
        assert fn(None, files, 2, (C.c_uint32 * 2)(0xFFFFFFFF, 1), c, v, d, None, res) == -1 and "32 bits" in why(), why()
        f3 = (_lib.PngPlanarIn * 3)()
        assert fn(None, f3, 3, (C.c_uint32 * 3)(0x80000000, 0x7FFFFFFF, 1), c, v, d, None, (_lib.DecodeResult * 3)()) == -1 and "32 bits" in why(), why()
        # every record the view call refuses, as the first, a middle and the last view of the call
        for crop, view, word in BAD:
            for at in range(3):
                records = [GOOD[0], GOOD[1], GOOD[2]]
                records[at] = (crop, view)
                files, cnt, c, v, d, res = _arrays(records, [2, 1])
                assert fn(None, files, 2, cnt, c, v, d, None, res) == -1 and word in why(), (crop, view, at, why())
        for crop, view in GOOD:
            files, cnt, c, v, d, res = _arrays([(crop, view)], [1])
            assert fn(None, files, 1, cnt, c, v, d, None, res) == -1 and "null/empty batch" in why(), (crop, view, why())
        # destination fields in `files`: the destinations are the fpng_amd_view_dest records
        for field, value in (("d_pixels", 4096), ("row_pitch", 8), ("row_pitch", -8), ("plane_pitch", 64), ("pixels_cap", 1)):
            files, cnt, c, v, d, res = _arrays([GOOD[0], GOOD[1], GOOD[2]], [2, 1])
            setattr(files[1], field, value)
            assert fn(None, files, 2, cnt, c, v, d, None, res) == -1 and "must be NULL / 0" in why(), (field, why())
    # the box: the same judgement of the records, and of the count
    box = _lib.Crop()
    _, _, c, v, _, _ = _arrays([GOOD[0], GOOD[1]], [2])
    assert lib.fpng_amd_views_source(None, v, 2, C.byref(box)) == -1 and "null" in why()
    assert lib.fpng_amd_views_source(c, None, 2, C.byref(box)) == -1 and "null" in why()
    assert lib.fpng_amd_views_source(c, v, 2, None) == -1 and "null" in why()
    assert lib.fpng_amd_views_source(c, v, 0, C.byref(box)) == -1 and "count of 0" in why()
    assert lib.fpng_amd_views_source(c, v, 2, C.byref(box)) == 0 and (box.x, box.y, box.w, box.h) == (0, 0, 96, 64)
    for crop, view, word in BAD:
        for at in range(2):
            records = [GOOD[0], GOOD[1]]
            records[at] = (crop, view)
            _, _, c, v, _, _ = _arrays(records, [2])
            assert lib.fpng_amd_views_source(c, v, 2, C.byref(box)) == -1 and word in why(), (crop, view, at, why())


@pytest.mark.parametrize("dtype,e", DTYPES)
def test_descriptor_nesting_and_broadcast(built_lib, dtype, e):
    """counts 1, 3, 2 from CPU tensor views (no device, as make_decode_batch_resize_view): the records lie file 0's first; full,
    window, filter and mirror once for all, per file, or per view; byte pitches and pixels_cap per view; `files` keeps empty
    destination fields"""
    canvas = torch.zeros(6, 4, 300, 400, dtype=dtype)
    crops = [[(5, 7, 9, 11)], [(250, 40, 13, 20), (0, 0, 600, 130), (61, 0, 7, 1)], [(0, 0, 600, 130), (10, 10, 500, 100)]]
    fulls = [(65, 17), [(13, 20), (256, 256), (9, 1)], (224, 224)]  # per file | per view | per file
    windows = [None, [(1, 2, 12, 18), (16, 16, 224, 224), (8, 0, 1, 1)], [(0, 0, 96, 96), None]]
    sizes = [[(65, 17)], [(12, 18), (224, 224), (1, 1)], [(96, 96), (224, 224)]]  # (w, h) of the destinations
    filters = ["bicubic", ["bilinear", fpng_amd.FILTER_BICUBIC, 0], "bilinear"]
    mirrors = [True, [False, True, True], [True, False]]
    chans = [3, 4, 3]
    flat_sizes = [s for per in sizes for s in per]
    slots = iter(range(6))
    outs = [[canvas[next(slots), :chans[i], 10:10 + oh, 20:20 + ow] for ow, oh in per] for i, per in enumerate(sizes)]
    pngs = [b"\x89PNG" + bytes(60)] * 3  # (host files: only their address and size are recorded)
    db = Encoder.make_decode_batch_views(pngs, crops, outs, fulls, windows, filters, mirror=mirrors, bottom_up=[False, True, False])
    assert isinstance(db, fpng_amd.DecodeBatchMultiView) and not isinstance(db, fpng_amd.DecodeBatchResizeView) and not db.device_data
    assert list(db.counts) == [1, 3, 2] and len(db.arr) == len(db.res) == 3 and len(db.crops) == len(db.views) == len(db.dests) == 6
    assert (db.fmt is None) == (dtype == torch.uint8)
    if db.fmt is not None:
        assert db.fmt.dtype == fpng_amd.FLOAT_DTYPES[dtype] and db.fmt.reserved == 0
    for i, r in enumerate(db.arr):
        assert (r.num_chans, r.size) == (chans[i], 64)
        assert (r.d_pixels, r.row_pitch, r.plane_pitch, r.pixels_cap) == (None, 0, 0, 0)
    want_views = [(65, 17, 0, 0, 65, 17, 1, 1), (13, 20, 1, 2, 12, 18, 0, 0), (256, 256, 16, 16, 224, 224, 1, 1), (9, 1, 8, 0, 1, 1, 1, 0),
                  (224, 224, 0, 0, 96, 96, 1, 0), (224, 224, 0, 0, 224, 224, 0, 0)]
    assert [(v.full_w, v.full_h, v.x, v.y, v.w, v.h, v.flags, v.filter) for v in db.views] == want_views
    assert [(c.x, c.y, c.w, c.h) for c in db.crops] == [c for per in crops for c in per]
    flat_outs = [t for per in outs for t in per]
    for k, (d, t, (ow, oh)) in enumerate(zip(db.dests, flat_outs, flat_sizes)):
        file = (0, 1, 1, 1, 2, 2)[k]
        rp = 400 * e if oh > 1 else 0
        first = t.data_ptr()
        assert d.plane_pitch == 300 * 400 * e
        assert (d.d_pixels, d.row_pitch) == ((first + (oh - 1) * rp, -rp) if file == 1 else (first, rp)), k  # (file 1: bottom-up)
        assert d.pixels_cap == (chans[file] - 1) * 300 * 400 * e + (oh - 1) * abs(rp) + ow * e
    # results(): a record per FILE, its views as the caller's own list
    got = db.results()
    assert len(got) == 3 and all(st == 0 and all(a is b for a, b in zip(ts, o)) for (st, ts, _), o in zip(got, outs))
    # one full size, window, filter and mirror flag for every view of every file
    batch = torch.zeros(5, 3, 96, 96, dtype=dtype)
    db = Encoder.make_decode_batch_views(pngs[:2], [crops[1][1:], crops[1]], [list(batch[:2]), list(batch[2:])], (224, 224), (8, 8, 96, 96), "bicubic", mirror=True)
    assert list(db.counts) == [2, 3]
    assert [(v.full_w, v.full_h, v.x, v.y, v.w, v.h, v.flags, v.filter) for v in db.views] == [(224, 224, 8, 8, 96, 96, 1, 1)] * 5
    assert [d.d_pixels for d in db.dests] == [batch[i].data_ptr() for i in range(5)]
    # order and bottom_up per view too: the second view of file 0 bottom-up, the third of file 1 with its planes in reverse
    db = Encoder.make_decode_batch_views(pngs[:2], [crops[1][1:], crops[1]], [list(batch[:2]), list(batch[2:])], (96, 96), bottom_up=[[False, True], False],
                                         order=["rgb", ["rgb", "rgb", "bgr"]])
    rp, pp = 96 * e, 96 * 96 * e
    assert [(d.d_pixels - batch[k].data_ptr(), d.row_pitch, d.plane_pitch) for k, d in enumerate(db.dests)] == [
        (0, rp, pp), (95 * rp, -rp, pp), (0, rp, pp), (0, rp, pp), (2 * pp, rp, -pp)]
    v = canvas[0, :3, :11, :9]
    two = [(0, 0, 90, 110), (1, 1, 90, 110)]
    for bad in (dict(crops=[[]], outs=[[]]),                                              # a file without a view
                dict(crops=[two], outs=[[v]]),                                            # two crops, one destination
                dict(crops=[two, two], outs=[[v, v]]),                                    # two files, one list of destinations
                dict(full=[(9, 11), (9, 11)]),                                            # a per-file list of another length (one file)
                dict(full=[[(9, 11)]]),                                                   # a per-view list of another length
                dict(window=[[None, None, None]]), dict(mirror=[[True]]), dict(filter=[["bicubic"] * 3]),
                dict(filter="nearest"), dict(window=(0, 0, 9, 12)),                       # an unknown filter; a destination that is not its window's size
                dict(outs=[[v, canvas[1, :4, :11, :9]]]),                                 # views of one file with different channel counts
                dict(outs=[[v, torch.zeros(3, 11, 9, dtype=torch.float16 if dtype != torch.float16 else torch.float32)]]),  # mixed dtypes
                dict(crops=[[(-1, 0, 9, 11), two[1]]]), dict(window=(-1, 0, 9, 11))):
        kw = dict(crops=[two], outs=[[v, v]], full=(9, 11))
        kw.update(bad)
        with pytest.raises(ValueError):
            Encoder.make_decode_batch_views(pngs[:len(kw["crops"])], **kw)
    if dtype == torch.uint8:
        for kw in ({"mean": (0.5,) * 3, "std": (0.5,) * 3}, {"scale": [1.0]}, {"bias": [0.0]}):
            with pytest.raises(ValueError):  # float arguments with uint8 destinations
                Encoder.make_decode_batch_views(pngs[:1], [two], [[v, v]], (9, 11), **kw)
    else:
        db = Encoder.make_decode_batch_views(pngs[:1], [two], [[v, v]], (9, 11), mean=(0.5,) * 3, std=(0.25,) * 3)
        assert db.fmt.scale[0] == pytest.approx(1 / (255 * 0.25)) and db.fmt.bias[2] == -2.0 and db.fmt.bias[3] == 0.0
