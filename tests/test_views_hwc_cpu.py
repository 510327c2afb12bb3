"""No-GPU tests of the CHANNELS-LAST views interface (fpng_amd_decode_batch(_device)_hwc_views): the exported symbols and the
fpng_amd_view_dest_hwc record, every call-level refusal -- none of which needs an encoder or a device -- dest_layout_hwc on CPU
tensor views, and the descriptor make_decode_batch_views_hwc builds, with the views call's nesting and broadcast rules."""
import ctypes as C

import pytest
import torch

import fpng_amd
from fpng_amd import _lib, dest_layout_hwc
from fpng_amd.api import Encoder

from test_resize_cpu import DTYPES
from test_resize_view_cpu import BAD, GOOD

NAMES = ("fpng_amd_decode_batch_hwc_views", "fpng_amd_decode_batch_device_hwc_views")


def test_entry_points_and_record(built_lib):
    lib = _lib.load()
    for name in NAMES:
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None
    assert lib.fpng_amd_abi_version() == 5  # (new entry points, the same ABI version)
    assert C.sizeof(_lib.ViewDestHwc) == 32
    assert {n: getattr(_lib.ViewDestHwc, n).offset for n, _ in _lib.ViewDestHwc._fields_} == {"d_pixels": 0, "row_pitch": 8, "pixel_elems": 16, "flags": 20, "pixels_cap": 24}
    assert _lib.HWC_REVERSED == 1
    assert C.sizeof(_lib.ViewDest) == 32 and C.sizeof(_lib.ResizeView) == 32 and C.sizeof(_lib.Crop) == 16 and C.sizeof(_lib.PngPlanarIn) == 48


def _arrays(records, counts, chans=3):
    """(files, view_count, crops, views, dests, results) with empty destination fields in `files`"""
    total, n = len(records), len(counts)
    files, cnt = (_lib.PngPlanarIn * n)(), (C.c_uint32 * n)(*counts)
    c, v, d = (_lib.Crop * total)(), (_lib.ResizeView * total)(), (_lib.ViewDestHwc * total)()
    for k, (crop, view) in enumerate(records):
        c[k].x, c[k].y, c[k].w, c[k].h = crop
        v[k].full_w, v[k].full_h, v[k].x, v[k].y, v[k].w, v[k].h, v[k].flags, v[k].filter = view
    for f in files:
        f.num_chans = chans
    return files, cnt, c, v, d, (_lib.DecodeResult * n)()


def test_call_level_refusals_need_no_encoder(built_lib):
    """Everything that needs no file is judged before the encoder is looked at: with a NULL encoder every call returns -1 and the
    message names the reason -- a bad argument its own, a good set only the missing encoder"""
    lib = _lib.load()
    fmt = _lib.FloatFormat()

    def why():
        return lib.fpng_amd_last_error().decode()

    for fn in (lib.fpng_amd_decode_batch_hwc_views, lib.fpng_amd_decode_batch_device_hwc_views):
        files, cnt, c, v, d, res = _arrays([GOOD[0], GOOD[1], GOOD[2]], [2, 1])
        good = [files, 2, cnt, c, v, d, None, res]
        assert fn(None, *good) == -1 and "null/empty batch" in why(), why()  # (nothing is at fault -- the batch has no encoder)
        assert fn(None, files, 2, cnt, c, v, d, C.byref(fmt), res) == -1 and "null/empty batch" in why(), why()
        # ---- everything the planar views call refuses ----
        for k in (0, 2, 3, 4, 5, 7):  # a null array
            args = list(good)
            args[k] = None
            assert fn(None, *args) == -1 and "null files, view_count, crops, views, dests or results" in why(), (k, why())
        for counts in ([0, 3], [3, 0], [0, 0]):  # a view_count of 0
            assert fn(None, files, 2, (C.c_uint32 * 2)(*counts), c, v, d, None, res) == -1 and "view_count of 0" in why(), (counts, why())
        assert fn(None, files, 2, (C.c_uint32 * 2)(0xFFFFFFFF, 1), c, v, d, None, res) == -1 and "32 bits" in why(), why()
        f3 = (_lib.PngPlanarIn * 3)()
        assert fn(None, f3, 3, (C.c_uint32 * 3)(0x80000000, 0x7FFFFFFF, 1), c, v, d, None, (_lib.DecodeResult * 3)()) == -1 and "32 bits" in why(), why()
        for crop, view, word in BAD:  # every record the view call refuses, as the first, a middle and the last view of the call
            for at in range(3):
                records = [GOOD[0], GOOD[1], GOOD[2]]
                records[at] = (crop, view)
                files, cnt, c, v, d, res = _arrays(records, [2, 1])
                assert fn(None, files, 2, cnt, c, v, d, None, res) == -1 and word in why(), (crop, view, at, why())
        for crop, view in GOOD:
            files, cnt, c, v, d, res = _arrays([(crop, view)], [1])
            assert fn(None, files, 1, cnt, c, v, d, None, res) == -1 and "null/empty batch" in why(), (crop, view, why())
        # ---- destination fields in `files`: the destinations are the fpng_amd_view_dest_hwc records ----
        for field, value in (("d_pixels", 4096), ("row_pitch", 8), ("row_pitch", -8), ("plane_pitch", 64), ("pixels_cap", 1)):
            files, cnt, c, v, d, res = _arrays([GOOD[0], GOOD[1], GOOD[2]], [2, 1])
            setattr(files[1], field, value)
            assert fn(None, files, 2, cnt, c, v, d, None, res) == -1 and "must be NULL / 0" in why(), (field, why())
        # ---- pixel_elems: 0, num_chans, or 4 with num_chans = 3 -- in the first, a middle and the last record ----
        for chans, bad, ok in ((3, (1, 2, 5, 6, 0xFFFFFFFF), (0, 3, 4)), (4, (1, 2, 3, 5), (0, 4))):
            for at in range(3):
                for px in bad:
                    files, cnt, c, v, d, res = _arrays([GOOD[0], GOOD[1], GOOD[2]], [2, 1], chans)
                    d[at].pixel_elems = px
                    assert fn(None, files, 2, cnt, c, v, d, None, res) == -1 and "pixel_elems" in why(), (chans, at, px, why())
                for px in ok:
                    files, cnt, c, v, d, res = _arrays([GOOD[0], GOOD[1], GOOD[2]], [2, 1], chans)
                    d[at].pixel_elems = px
                    assert fn(None, files, 2, cnt, c, v, d, None, res) == -1 and "null/empty batch" in why(), (chans, at, px, why())
        # (num_chans is the FILE's: file 0 with 4 channels and file 1 with 3 -- 3 is refused in file 0's records only)
        files, cnt, c, v, d, res = _arrays([GOOD[0], GOOD[1], GOOD[2]], [2, 1])
        files[0].num_chans = 4
        d[2].pixel_elems = 3
        assert fn(None, files, 2, cnt, c, v, d, None, res) == -1 and "null/empty batch" in why(), why()
        d[1].pixel_elems = 3
        assert fn(None, files, 2, cnt, c, v, d, None, res) == -1 and "pixel_elems" in why(), why()
        # ---- unknown flag bits ----
        for at in range(3):
            for flags in (2, 3, 0x80000000, 0xFFFFFFFE):
                files, cnt, c, v, d, res = _arrays([GOOD[0], GOOD[1], GOOD[2]], [2, 1])
                d[at].flags = flags
                assert fn(None, files, 2, cnt, c, v, d, None, res) == -1 and "flags" in why(), (at, flags, why())
            files, cnt, c, v, d, res = _arrays([GOOD[0], GOOD[1], GOOD[2]], [2, 1])
            d[at].flags = _lib.HWC_REVERSED
            assert fn(None, files, 2, cnt, c, v, d, None, res) == -1 and "null/empty batch" in why(), (at, why())


@pytest.mark.parametrize("dtype,e", DTYPES)
def test_dest_layout_hwc_accepts(dtype, e):
    code = None if dtype == torch.uint8 else fpng_amd.FLOAT_DTYPES[dtype]
    hwc = torch.zeros(30, 40, 3, dtype=dtype)
    assert dest_layout_hwc(hwc) == (hwc.data_ptr(), 120 * e, 3, 0, code)
    assert dest_layout_hwc(hwc, "bgr") == (hwc.data_ptr(), 120 * e, 3, 1, code)
    assert dest_layout_hwc(hwc, "RGB", bottom_up=True) == (hwc.data_ptr() + 29 * 120 * e, -120 * e, 3, 0, code)
    rgba = torch.zeros(30, 40, 4, dtype=dtype)
    assert dest_layout_hwc(rgba) == dest_layout_hwc(rgba, "rgb") == dest_layout_hwc(rgba, "rgba") == (rgba.data_ptr(), 160 * e, 4, 0, code)
    assert dest_layout_hwc(rgba, "abgr") == (rgba.data_ptr(), 160 * e, 4, 1, code)
    assert dest_layout_hwc(rgba[..., :3]) == (rgba.data_ptr(), 160 * e, 4, 0, code)  # (4-element pixels under 3 channels)
    assert dest_layout_hwc(rgba[..., :3], "bgr", True) == (rgba.data_ptr() + 29 * 160 * e, -160 * e, 4, 1, code)
    crop = hwc[5:25, 7:17]  # a crop keeps the row stride
    assert dest_layout_hwc(crop) == (hwc.data_ptr() + (5 * 120 + 7 * 3) * e, 120 * e, 3, 0, code)
    assert dest_layout_hwc(rgba[4:9, 8:12, :3]) == (rgba.data_ptr() + (4 * 160 + 8 * 4) * e, 160 * e, 4, 0, code)
    assert dest_layout_hwc(hwc[3:4]) == (hwc.data_ptr() + 3 * 120 * e, 0, 3, 0, code)  # (one row: no pitch)
    assert dest_layout_hwc(hwc[3:4], bottom_up=True) == (hwc.data_ptr() + 3 * 120 * e, 0, 3, 0, code)
    assert dest_layout_hwc(hwc[:, 9:10]) == (hwc.data_ptr() + 27 * e, 120 * e, 3, 0, code)  # (one column: any stride(1))
    assert dest_layout_hwc(hwc[::2]) == (hwc.data_ptr(), 240 * e, 3, 0, code)  # (padded rows)
    # the one-liner the call exists for: file i's destination in a channels-last batch
    x = torch.empty((4, 3, 24, 32), dtype=dtype).contiguous(memory_format=torch.channels_last)
    for i in range(4):
        v = x[i].permute(1, 2, 0)
        assert tuple(v.shape) == (24, 32, 3) and v.stride() == (96, 3, 1)
        assert dest_layout_hwc(v) == (x.data_ptr() + i * 24 * 32 * 3 * e, 96 * e, 3, 0, code)
    x4 = torch.empty((2, 4, 8, 8), dtype=dtype).contiguous(memory_format=torch.channels_last)
    assert dest_layout_hwc(x4[1].permute(1, 2, 0)) == (x4.data_ptr() + 256 * e, 32 * e, 4, 0, code)
    assert dest_layout_hwc(x4[1, :3].permute(1, 2, 0)) == (x4.data_ptr() + 256 * e, 32 * e, 4, 0, code)


def test_dest_layout_hwc_refuses():
    hwc, rgba, chw = torch.zeros(30, 40, 3, dtype=torch.uint8), torch.zeros(30, 40, 4, dtype=torch.float16), torch.zeros(3, 30, 40, dtype=torch.uint8)
    for bad in (chw.permute(1, 2, 0),                             # CHW-strided: the planar calls' layout
                torch.zeros(4, 30, 40).permute(1, 2, 0),
                torch.zeros(30, 40, 5, dtype=torch.uint8)[..., :3],   # stride(1) of 5
                torch.zeros(30, 40, 5, dtype=torch.uint8)[..., :4],
                torch.zeros(30, 40, 8, dtype=torch.uint8)[..., :4],
                torch.zeros(30, 40, 6, dtype=torch.uint8)[..., ::2],  # stride(2) of 2
                rgba[..., 1:],                                         # a view that starts inside the pixel
                torch.zeros(30, 40, 4, dtype=torch.uint8)[..., 1:],
                hwc[:1].expand(30, 40, 3),                             # stride 0
                hwc.as_strided((30, 40, 3), (119, 3, 1)),              # overlapping rows
                hwc[:, :1].expand(30, 40, 3),                          # stride(1) of 0
                torch.zeros(30, 40, 2, dtype=torch.uint8), torch.zeros(30, 40, 1, dtype=torch.uint8), torch.zeros(30, 40, 5, dtype=torch.uint8),
                torch.zeros(30, 40, 3, dtype=torch.float64), torch.zeros(30, 40, 3, dtype=torch.int8), torch.zeros(30, 40, 3, dtype=torch.int32),
                torch.zeros(30, 40, dtype=torch.uint8), torch.zeros(2, 30, 40, 3, dtype=torch.uint8), torch.zeros(0, 40, 3, dtype=torch.uint8),
                hwc.numpy(), None):
        with pytest.raises(ValueError):
            dest_layout_hwc(bad)
    # (a row ends at its last WRITTEN element: with 4-element pixels under 3 channels a row stride of 39 * 4 + 3 is no overlap)
    assert dest_layout_hwc(torch.zeros(30, 160, dtype=torch.uint8).as_strided((30, 40, 3), (159, 4, 1)))[1:4] == (159, 4, 0)
    with pytest.raises(ValueError):
        dest_layout_hwc(torch.zeros(30, 160, dtype=torch.uint8).as_strided((30, 40, 3), (158, 4, 1)))  # (one below the row's span)
    for t, order in ((hwc, "rgba"), (hwc, "abgr"), (hwc, "brg"), (hwc, "xrgb"), (rgba, "bgr"), (rgba, "bgra"), (rgba, "argb"), (rgba, "rgbx")):
        with pytest.raises(ValueError):
            dest_layout_hwc(t, order)


@pytest.mark.parametrize("dtype,e", DTYPES)
def test_descriptor_nesting_and_broadcast(built_lib, dtype, e):
    """counts 1, 3, 2 from CPU tensor views (no device): the records lie file 0's first; full, window, filter and mirror once for
    all, per file, or per view; byte pitches, pixel_elems, flags and pixels_cap per view; `files` keeps empty destination fields"""
    canvas = torch.zeros(6, 300, 400, 4, dtype=dtype)
    crops = [[(5, 7, 9, 11)], [(250, 40, 13, 20), (0, 0, 600, 130), (61, 0, 7, 1)], [(0, 0, 600, 130), (10, 10, 500, 100)]]
    fulls = [(65, 17), [(13, 20), (256, 256), (9, 1)], (224, 224)]  # per file | per view | per file
    windows = [None, [(1, 2, 12, 18), (16, 16, 224, 224), (8, 0, 1, 1)], [(0, 0, 96, 96), None]]
    sizes = [[(65, 17)], [(12, 18), (224, 224), (1, 1)], [(96, 96), (224, 224)]]  # (w, h) of the destinations
    filters = ["bicubic", ["bilinear", fpng_amd.FILTER_BICUBIC, 0], "bilinear"]
    mirrors = [True, [False, True, True], [True, False]]
    chans = [3, 4, 3]
    flat_sizes = [s for per in sizes for s in per]
    slots = iter(range(6))
    outs = [[canvas[next(slots), 10:10 + oh, 20:20 + ow, :chans[i]] for ow, oh in per] for i, per in enumerate(sizes)]
    pngs = [b"\x89PNG" + bytes(60)] * 3  # (host files: only their address and size are recorded)
    db = Encoder.make_decode_batch_views_hwc(pngs, crops, outs, fulls, windows, filters, mirror=mirrors, bottom_up=[False, True, False], order=["bgr", "rgb", "rgb"])
    assert isinstance(db, fpng_amd.DecodeBatchMultiViewHwc) and not isinstance(db, fpng_amd.DecodeBatchMultiView) and not db.device_data
    assert list(db.counts) == [1, 3, 2] and len(db.arr) == len(db.res) == 3 and len(db.crops) == len(db.views) == len(db.dests) == 6
    assert isinstance(db.dests[0], _lib.ViewDestHwc)
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
        rp = 1600 * e if oh > 1 else 0
        first = t.data_ptr()
        assert (d.d_pixels, d.row_pitch) == ((first + (oh - 1) * rp, -rp) if file == 1 else (first, rp)), k  # (file 1: bottom-up)
        assert (d.pixel_elems, d.flags) == (4 if ow > 1 else chans[file], 1 if file == 0 else 0), k  # (4-element pixels; one column: the channels)
        assert d.pixels_cap == (oh - 1) * abs(rp) + ((ow - 1) * d.pixel_elems + chans[file]) * e
    got = db.results()  # a record per FILE, its views as the caller's own list
    assert len(got) == 3 and all(st == 0 and all(a is b for a, b in zip(ts, o)) for (st, ts, _), o in zip(got, outs))
    # one full size, window, filter and mirror flag for every view of every file; contiguous HWC destinations
    batch = torch.zeros(5, 96, 96, 3, dtype=dtype)
    db = Encoder.make_decode_batch_views_hwc(pngs[:2], [crops[1][1:], crops[1]], [list(batch[:2]), list(batch[2:])], (224, 224), (8, 8, 96, 96), "bicubic", mirror=True)
    assert list(db.counts) == [2, 3]
    assert [(v.full_w, v.full_h, v.x, v.y, v.w, v.h, v.flags, v.filter) for v in db.views] == [(224, 224, 8, 8, 96, 96, 1, 1)] * 5
    assert [(d.d_pixels, d.row_pitch, d.pixel_elems, d.flags, d.pixels_cap) for d in db.dests] == [(batch[i].data_ptr(), 288 * e, 3, 0, 96 * 288 * e) for i in range(5)]
    # order and bottom_up per view too; the destinations of a channels-last batch
    x = torch.zeros(5, 3, 96, 96, dtype=dtype).contiguous(memory_format=torch.channels_last)
    views = [x[i].permute(1, 2, 0) for i in range(5)]
    db = Encoder.make_decode_batch_views_hwc(pngs[:2], [crops[1][1:], crops[1]], [views[:2], views[2:]], (96, 96), bottom_up=[[False, True], False],
                                             order=["rgb", ["rgb", "rgb", "bgr"]])
    rp = 288 * e
    assert [(d.d_pixels - x[k].data_ptr(), d.row_pitch, d.pixel_elems, d.flags) for k, d in enumerate(db.dests)] == [
        (0, rp, 3, 0), (95 * rp, -rp, 3, 0), (0, rp, 3, 0), (0, rp, 3, 0), (0, rp, 3, 1)]
    v = canvas[0, :11, :9, :3]
    two = [(0, 0, 90, 110), (1, 1, 90, 110)]
    for bad in (dict(crops=[[]], outs=[[]]),                                              # a file without a view
                dict(crops=[two], outs=[[v]]),                                            # two crops, one destination
                dict(crops=[two, two], outs=[[v, v]]),                                    # two files, one list of destinations
                dict(full=[(9, 11), (9, 11)]),                                            # a per-file list of another length (one file)
                dict(full=[[(9, 11)]]),                                                   # a per-view list of another length
                dict(window=[[None, None, None]]), dict(mirror=[[True]]), dict(filter=[["bicubic"] * 3]),
                dict(filter="nearest"), dict(window=(0, 0, 9, 12)),                       # an unknown filter; a destination that is not its window's size
                dict(outs=[[v, canvas[1, :11, :9, :4]]]),                                 # views of one file with different channel counts
                dict(outs=[[v, torch.zeros(11, 9, 3, dtype=torch.float16 if dtype != torch.float16 else torch.float32)]]),  # mixed dtypes
                dict(outs=[[v, torch.zeros(3, 11, 9, dtype=dtype)]]),                     # a planar destination
                dict(order="rgba"),
                dict(crops=[[(-1, 0, 9, 11), two[1]]]), dict(window=(-1, 0, 9, 11))):
        kw = dict(crops=[two], outs=[[v, v]], full=(9, 11))
        kw.update(bad)
        with pytest.raises(ValueError):
            Encoder.make_decode_batch_views_hwc(pngs[:len(kw["crops"])], **kw)
    if dtype == torch.uint8:
        for kw in ({"mean": (0.5,) * 3, "std": (0.5,) * 3}, {"scale": [1.0]}, {"bias": [0.0]}):
            with pytest.raises(ValueError):  # float arguments with uint8 destinations
                Encoder.make_decode_batch_views_hwc(pngs[:1], [two], [[v, v]], (9, 11), **kw)
    else:
        db = Encoder.make_decode_batch_views_hwc(pngs[:1], [two], [[v, v]], (9, 11), mean=(0.5,) * 3, std=(0.25,) * 3)
        assert db.fmt.scale[0] == pytest.approx(1 / (255 * 0.25)) and db.fmt.bias[2] == -2.0 and db.fmt.bias[3] == 0.0
