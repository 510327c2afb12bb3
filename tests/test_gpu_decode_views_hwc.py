"""GPU decoder of several resized views of each file into CHANNELS-LAST destinations (-m gpu; fpng_amd_decode_batch_hwc_views /
fpng_amd_decode_batch_device_hwc_views: the views call's crop stage, then dec_resize_hwc_kernel -- one workgroup per tile, all
planes, whole pixels written as contiguous runs): uint8 and the three float dtypes, three and four channels, both filters,
mirrors, every destination kind, host and device files.

Expected values never come from the library: the pixels are the REFERENCE's decoder's (judge()), sliced to each view's crop, resized
WHOLE and sliced to the window by resize_view_model.py, looked up in test_gpu_decode_float's table for the float dtypes and laid
out as (h, w, c).  Every call decodes into ONE sentinel-filled buffer that is compared WHOLE and bit for bit, so the fourth element
of 4-element pixels under a 3-channel view, pitch padding and everything around a view must still hold the sentinel.

The shapes are the views tests' (600 x 130, 257 x 49, 64 x 97 and 1 x 1 files) plus one window of 129 x 33 samples: three tile
columns and three tile rows -- more rows of tiles' samples than waves -- with a partial last tile on both axes, plain and mirrored
(the mirror's index across a tile border)."""
import numpy as np
import pytest

from test_gpu_decode import UNDECIDED, _device_files
from test_gpu_decode_float import CONSTS
from test_gpu_decode_layouts import SENTINEL, _damaged_files, _header_dims
from test_gpu_decode_resize import BITS, CROP_OUTSIDE, DTYPES, ELEM, _elements, enc, files  # noqa: F401  (enc, files: fixtures)
from test_gpu_decode_views import _mixed_counts
from test_gpu_resize_view import _window, model  # noqa: F401  (model: a fixture)
import resize_view_model as VM

pytestmark = pytest.mark.gpu

KINDS = ["tight", "pad256", "odd", "bottom_up", "reversed", "px4"]
INVALID_ARG, BUFFER_TOO_SMALL = -1, -4


class _Region:
    """a view's destination inside one sentinel-filled buffer, in BYTES: a margin, h rows `rp` bytes apart of w pixels of P elements
    of e bytes, c of them written, a margin.  odd: an odd pitch from an odd byte (uint8; else tight); px4: P = 4 under c = 3 (c = 4:
    tight)"""

    def __init__(self, off, w, h, c, kind, e):
        if (kind == "odd" and e != 1) or (kind == "px4" and c != 3):
            kind = "tight"
        self.w, self.h, self.c, self.kind, self.e = w, h, c, kind, e
        self.P = 4 if kind == "px4" else c
        self.rp = w * self.P * e + {"pad256": 256}.get(kind, 0)
        if kind == "odd":
            self.rp += 7 - (self.rp & 1)
        self.front = 64 + (1 if kind == "odd" else 0)
        self.off, self.lo = off, off + self.front
        self.span = ((w - 1) * self.P + c) * e  # a row, up to its last written byte
        self.size = (self.front + (h - 1) * self.rp + self.span + 64 + 15) & ~15  # (a region starts on a 16-byte boundary)

    def order(self):
        return ("bgr" if self.c == 3 else "abgr") if self.kind == "reversed" else ("rgb" if self.c == 3 else "rgba")

    def view(self, typed):  # the (h, w, c) tensor view a caller holds (rows in memory order)
        e = self.e
        return typed.as_strided((self.h, self.w, self.c), (self.rp // e, self.P, 1), self.lo // e)

    def row(self, y):  # the first byte of the image's row y
        return self.lo + ((self.h - 1 - y) if self.kind == "bottom_up" else y) * self.rp

    def put(self, exp, px):  # px (h, w, c) element bits in the FILE's channel order into the expected BYTES
        e = self.e
        at = np.arange(self.w) * self.P * e
        for ch in range(self.c):
            k = (self.c - 1 - ch) if self.kind == "reversed" else ch
            by = np.ascontiguousarray(px[:, :, ch]).astype(BITS[e]).view(np.uint8).reshape(self.h, self.w, e)  # (little endian)
            for y in range(self.h):
                for b in range(e):
                    exp[self.row(y) + k * e + b + at] = by[y, :, b]

    def spans(self):
        return [(self.row(y), self.row(y) + self.span) for y in range(self.h)]


def _decode(enc, pngs, plan, dtype, device, dev=None, consts=CONSTS[0]):  # noqa: F811
    """plan: per file (c, [(crop, full, window, filter, mirror, kind)]).  ONE call into ONE sentinel-filled buffer: (results, the
    buffer's bytes afterwards, the tensors per file, the regions in the records' order)"""
    import torch
    e = ELEM[dtype]
    regs, off = [], 0
    for c, views in plan:
        for _, full, window, _, _, kind in views:
            r = _Region(off, *_window(full, window)[2:], c, kind, e)
            regs.append(r)
            off += r.size
    buf = torch.full((off,), SENTINEL, dtype=torch.uint8, device="cuda")
    typed = buf.view(getattr(torch, dtype))
    it = iter(regs)
    per = [[next(it) for _ in views] for _, views in plan]
    outs = [[r.view(typed) for r in rs] for rs in per]
    kw = {} if dtype == "uint8" else {"scale": consts[0], "bias": consts[1]}
    args = ([[v[0] for v in views] for _, views in plan], outs, [[v[1] for v in views] for _, views in plan], [[v[2] for v in views] for _, views in plan],
            [[v[3] for v in views] for _, views in plan])
    kw.update(mirror=[[v[4] for v in views] for _, views in plan], order=[[r.order() for r in rs] for rs in per], bottom_up=[[r.kind == "bottom_up" for r in rs] for rs in per])
    if device:
        got = enc.decode_device_views_hwc(dev if dev is not None else _device_files(pngs, shift=1), *args, **kw)
    else:
        got = enc.decode_batch_views_hwc(pngs, *args, **kw)
    torch.cuda.synchronize()
    return got, buf.cpu().numpy(), outs, regs


def _sources(model, idx, plan, dtype, skip=()):  # noqa: F811
    """the (oh, ow, c) elements of every view, in the records' order (None for the views of the files in `skip`)"""
    return [None if n in skip else _elements(model.view(idx[n], crop, full, window, f), c, dtype, m)
            for n, (c, views) in enumerate(plan) for crop, full, window, f, m, _ in views]


def _expect(regs, total, sources):
    exp = np.full(total, SENTINEL, dtype=np.uint8)
    for r, src in zip(regs, sources):
        if src is not None:
            r.put(exp, src)
    return exp


def _first_difference(host, exp, regs):
    bad = np.nonzero(host != exp)[0]
    if not bad.size:
        return None
    return (bad.size, int(bad[0]), hex(int(host[bad[0]])), hex(int(exp[bad[0]])),
            [(i, r.w, r.h, r.c, r.kind, int(bad[0]) - r.lo) for i, r in enumerate(regs) if r.off <= bad[0] < r.off + r.size])


def _run(enc, files, model, idx, plan, dtype, device, **kw):  # noqa: F811
    got, host, outs, regs = _decode(enc, [files.pngs[i] for i in idx], plan, dtype, device, **kw)
    assert len(got) == len(idx)
    for n, (i, (st, views, cf)) in enumerate(zip(idx, got)):
        assert st == 0 and cf == files.chans[i] and len(views) == len(outs[n]) and all(a is b for a, b in zip(views, outs[n])), (n, i, st, cf)
    diff = _first_difference(host, _expect(regs, host.size, _sources(model, idx, plan, dtype)), regs)
    assert diff is None, (dtype, device, diff)
    return regs


def _all_views(files, i, filter, k0=0):  # noqa: F811
    """every view of file i's size as (crop, full, window, filter, mirror, kind): mirror flags alternating, destination kinds dealt"""
    return [(crop, full, window, filter if filter in fs else fs[0], bool((k0 + k + (k0 + k) // len(KINDS)) & 1), KINDS[(k0 + k) % len(KINDS)])  # (every kind both ways)
            for k, (crop, full, window, fs) in enumerate(VM.VIEWS[files.dims[i]])]


@pytest.mark.parametrize("filter", VM.FILTERS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", [3, 4])
def test_all_views_of_a_size_at_once_device_files(enc, files, model, c, dtype, filter):  # noqa: F811
    """every file with ALL the views of its size -- ten for a 600 x 130 file -- in ONE call into ONE buffer that is compared whole"""
    idx = list(range(len(files.pngs)))
    assert sum(d == (600, 130) for d in files.dims) == 6 and len(VM.VIEWS[(600, 130)]) == 10
    regs = _run(enc, files, model, idx, [(c, _all_views(files, i, filter, k0=i + c)) for i in idx], dtype, True)
    want = set(KINDS) - ({"odd"} if dtype != "uint8" else set()) - ({"px4"} if c == 4 else set())
    assert {r.kind for r in regs} == want


@pytest.mark.parametrize("c,dtype,filter", [(3, "uint8", "bicubic"), (4, "bfloat16", "bilinear"), (3, "float32", "bicubic")])
def test_all_views_of_a_size_at_once_host_files(enc, files, model, c, dtype, filter):  # noqa: F811
    """the same through fpng_amd_decode_batch_hwc_views (files in host memory), for a subset"""
    idx = list(range(len(files.pngs)))[::2]
    _run(enc, files, model, idx, [(c, _all_views(files, i, filter, k0=2 * i + c)) for i in idx], dtype, False)


@pytest.mark.parametrize("filter", VM.FILTERS)
@pytest.mark.parametrize("dtype", ["uint8", "float16"])
def test_tile_borders_plain_and_mirrored(enc, files, model, dtype, filter):  # noqa: F811
    """a window of 129 x 33 samples -- three tile columns and rows, the last of each partial -- plain and MIRRORED, and the 65 x 17
    and 2 x 194 windows mirrored, over every destination kind: the mirror's index is taken over the window, not the tile"""
    whole = (0, 0, 600, 130)
    i600 = [i for i, d in enumerate(files.dims) if d == (600, 130)]
    i64 = [i for i, d in enumerate(files.dims) if d == (64, 97)]
    assert len(i600) == 6 and len(i64) == 2
    idx, plan = [], []
    for n, i in enumerate(i600):
        c = 3 + (n & 1)
        views = [(whole, (300, 65), (0, 0, 129, 33), filter, False, KINDS[n % len(KINDS)]), (whole, (300, 65), (0, 0, 129, 33), filter, True, KINDS[(n + 1) % len(KINDS)]),
                 (whole, (300, 65), (235, 48, 65, 17), filter, True, KINDS[(n + 2) % len(KINDS)])]
        idx.append(i), plan.append((c, views))
    for n, i in enumerate(i64):
        idx.append(i), plan.append((4 - n, [((0, 0, 64, 97), (128, 194), (63, 0, 2, 194), filter, True, KINDS[(2 + 3 * n) % len(KINDS)])]))
    _run(enc, files, model, idx, plan, dtype, True)


def _hwc_kinds(plan):
    """_mixed_counts' plan with this file's destination kinds dealt in the place of the planar ones"""
    k = 0
    out = []
    for c, views in plan:
        out.append((c, [v[:5] + (KINDS[(k + j) % len(KINDS)],) for j, v in enumerate(views)]))
        k += len(views)
    return out


@pytest.mark.parametrize("device", [False, True])
def test_mixed_counts_in_one_batch(enc, files, model, device):  # noqa: F811
    """counts 1, 10, 2, 1 over a stored 4-channel, a 2-pass 4-channel, a stored 3-channel and a 1-pass 3-channel file, into 4, 3, 4 and
    3 channels: alpha dropped, A = 255 (fmaf(255, ...)) added, tile counts and channel counts changing from record to record"""
    for k0, dtype in ((0, "float16"), (3, "uint8")):
        idx, plan = _mixed_counts(files, k0)
        assert [files.chans[i] for i in idx] == [4, 4, 3, 3] and [c for c, _ in plan] == [4, 3, 4, 3]
        _run(enc, files, model, idx, _hwc_kinds(plan), dtype, device)


def test_the_channels_last_batch(enc, files, model):  # noqa: F811
    """x: (n, 3, 64, 64) f16 in torch.channels_last; file i's destination is x[i].permute(1, 2, 0).  Afterwards x[i] holds the
    model's (c, h, w) elements and x is still contiguous in channels_last"""
    import torch
    idx = [i for i, d in enumerate(files.dims) if d == (600, 130)]
    n = len(idx)
    crops = [(3 * k, k, 500 + 9 * k, 100 + 5 * k) for k in range(n)]
    filters = [VM.FILTERS[k & 1] for k in range(n)]
    x = torch.full((n, 3, 64, 64), -7.0, dtype=torch.float16, device="cuda").contiguous(memory_format=torch.channels_last)
    assert x.stride() == (64 * 64 * 3, 1, 64 * 3, 3)
    outs = [[x[k].permute(1, 2, 0)] for k in range(n)]
    got = enc.decode_device_views_hwc(_device_files([files.pngs[i] for i in idx], shift=1), [[c] for c in crops], outs, (64, 64), None, [[f] for f in filters],
                                      mirror=[[bool(k & 1)] for k in range(n)], scale=CONSTS[0][0], bias=CONSTS[0][1])
    torch.cuda.synchronize()
    assert [st for st, _, _ in got] == [0] * n
    assert x.is_contiguous(memory_format=torch.channels_last) and not x.is_contiguous()
    host = x.cpu()
    for k, i in enumerate(idx):
        want = _elements(model.view(i, crops[k], (64, 64), None, filters[k]), 3, "float16", bool(k & 1))  # (h, w, c) bits
        assert np.array_equal(host[k].view(torch.int16).numpy().view(np.uint16), want.transpose(2, 0, 1)), k


@pytest.mark.parametrize("c", [3, 4])
def test_the_identity_is_a_plain_hwc_float_crop(enc, files, c):  # noqa: F811
    """full = the crop's size with the whole window, f32: the reference decoder's pixels of that crop through the float table"""
    import torch
    cases = [(i, (w // 3, h // 4, min(200, w - w // 3), min(70, h - h // 4))) for i, (w, h) in list(enumerate(files.dims))[::2]]  # (the 1 x 1 file: itself)
    outs = [[torch.full((ch, cw, c), -3.0, dtype=torch.float32, device="cuda")] for _, (_, _, cw, ch) in cases]
    got = enc.decode_device_views_hwc(_device_files([files.pngs[i] for i, _ in cases]), [[crop] for _, crop in cases], outs, [(crop[2], crop[3]) for _, crop in cases],
                                      scale=CONSTS[0][0], bias=CONSTS[0][1])
    torch.cuda.synchronize()
    for (i, (x, y, cw, ch)), (st, ts, _), o in zip(cases, got, outs):
        want = _elements(files.planes[i][:, y:y + ch, x:x + cw], c, "float32", False)
        assert st == 0 and ts[0] is o[0]
        assert np.array_equal(o[0].cpu().view(torch.int32).numpy().view(np.uint32), want), (i, x, y, cw, ch)


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("dtype", ["uint8", "float16"])
def test_statuses(enc, files, model, dtype, device):  # noqa: F811
    """a file one of whose crops leaves the image (67) and a damaged file next to good ones: the statuses are the planar views
    call's, the two files' regions are all sentinel, every other file is exact"""
    import torch
    damaged = None
    for p in _damaged_files():
        w, h = _header_dims(p)
        if not (2 <= w <= 600 and 2 <= h <= 600):
            continue
        dviews = [((0, h - 2, w, 2), (max(w // 3, 1), 3), None, "bicubic", True, "odd"), ((0, 0, min(w, 5), 1), (3, 3), (1, 1, 2, 2), "bilinear", False, "tight")]
        nest = [[[v[k] for v in dviews]] for k in range(4)]
        planar = [[torch.full((3,) + _window(v[1], v[2])[:1:-1], SENTINEL, dtype=torch.uint8, device="cuda") for v in dviews]]
        (st, _, _), = enc.decode_batch_views([p], nest[0], planar, nest[1], nest[2], nest[3])
        torch.cuda.synchronize()
        # (a file that is refused before its resize is launched -- the planar call leaves its destinations alone: so must this one)
        if st not in (0, UNDECIDED) and all(bool((t == SENTINEL).all()) for t in planar[0]):
            damaged = (p, dviews, st)
            break
    assert damaged is not None
    idx, plan = _mixed_counts(files, 1)
    plan = _hwc_kinds(plan)
    outside = [plan[2][1][0], ((files.dims[2][0] - 1, 0, 2, 1), (7, 5), (1, 1, 5, 3), "bicubic", False, "pad256"), plan[2][1][1]]
    plan[2] = (plan[2][0], outside)
    plan.append((3, damaged[1]))
    pngs = [files.pngs[i] for i in idx] + [damaged[0]]
    got, host, outs, regs = _decode(enc, pngs, plan, dtype, device)
    assert [st for st, _, _ in got] == [0, 0, CROP_OUTSIDE, 0, damaged[2]] and got[2][1] is None and got[4][1] is None
    # (the rejected files' sources are None: their regions are expected to be all sentinel)
    exp = _expect(regs, host.size, _sources(model, idx + [None], plan, dtype, skip=(2, 4)))
    assert _first_difference(host, exp, regs) is None, _first_difference(host, exp, regs)


@pytest.mark.parametrize("dtype", ["uint8", "bfloat16"])
def test_the_planar_views_call_permuted_is_equal(enc, files, dtype):  # noqa: F811
    """secondary cross-check: the same plan through decode_device_views, permuted to (h, w, c), bit for bit"""
    import torch
    idx, plan = _mixed_counts(files, 2)
    dev = _device_files([files.pngs[i] for i in idx], shift=3)
    nest = [[[v[k] for v in views] for _, views in plan] for k in range(5)]
    kw = {} if dtype == "uint8" else {"scale": CONSTS[1][0], "bias": CONSTS[1][1]}
    td = getattr(torch, dtype)
    shapes = [[_window(full, window)[:1:-1] for _, full, window, *_ in views] for _, views in plan]
    planar = [[torch.zeros((c,) + s, dtype=td, device="cuda") for s in ss] for (c, _), ss in zip(plan, shapes)]
    hwc = [[torch.ones(s + (c,), dtype=td, device="cuda") for s in ss] for (c, _), ss in zip(plan, shapes)]
    a = enc.decode_device_views(dev, nest[0], planar, nest[1], nest[2], nest[3], mirror=nest[4], **kw)
    b = enc.decode_device_views_hwc(dev, nest[0], hwc, nest[1], nest[2], nest[3], mirror=nest[4], **kw)
    torch.cuda.synchronize()
    assert [(st, cf) for st, _, cf in a] == [(st, cf) for st, _, cf in b] == [(0, files.chans[i]) for i in idx]
    for ps, hs in zip(planar, hwc):
        for p, h in zip(ps, hs):
            assert torch.equal(p.permute(1, 2, 0).contiguous().view(torch.uint8), h.view(torch.uint8))


def test_call_level_errors_leave_the_buffer_untouched(enc, files):  # noqa: F811
    """pixels_cap one byte short, |row_pitch| one below the row span, a misaligned d_pixels under fmt: each its error, nothing written"""
    import torch
    import fpng_amd
    i = [k for k, d in enumerate(files.dims) if d == (600, 130)][0]
    dev = _device_files([files.pngs[i], files.pngs[i]])
    crops, full = [[(0, 0, 600, 130)], [(10, 10, 300, 100), (0, 0, 64, 64)]], (40, 20)

    def descriptor(dtype):
        buf = torch.full((3, 20, 40, 3), SENTINEL, dtype=torch.uint8, device="cuda") if dtype == torch.uint8 else \
            torch.full((3 * 20 * 40 * 3 * 2,), SENTINEL, dtype=torch.uint8, device="cuda").view(torch.float16).view(3, 20, 40, 3)
        return buf, enc.make_decode_batch_views_hwc(dev, crops, [[buf[0]], [buf[1], buf[2]]], full)

    def refused(db, code, buf):
        with pytest.raises(fpng_amd.FpngAmdError) as err:
            enc.decode_device_views_hwc(db)
        torch.cuda.synchronize()
        assert err.value.code == code, err.value
        assert bool((buf.view(torch.uint8) == SENTINEL).all())

    for dtype, e in ((torch.uint8, 1), (torch.float16, 2)):
        span = 40 * 3 * e
        buf, db = descriptor(dtype)
        assert [(d.row_pitch, d.pixel_elems, d.pixels_cap) for d in db.dests] == [(span, 3, 20 * span)] * 3
        db.dests[2].pixels_cap -= 1
        refused(db, BUFFER_TOO_SMALL, buf)
        buf, db = descriptor(dtype)
        db.dests[1].row_pitch = span - e  # (a multiple of the element size: the pitch rule itself refuses it)
        refused(db, INVALID_ARG, buf)
        buf, db = descriptor(dtype)
        db.dests[1].row_pitch = -(span - e)
        refused(db, INVALID_ARG, buf)
        buf, db = descriptor(dtype)
        db.dests[0].d_pixels = None
        refused(db, BUFFER_TOO_SMALL, buf)
    buf, db = descriptor(torch.float16)
    db.dests[2].d_pixels += 1
    refused(db, INVALID_ARG, buf)
    buf, db = descriptor(torch.float16)
    db.dests[0].row_pitch += 1
    refused(db, INVALID_ARG, buf)
    buf, db = descriptor(torch.float16)  # (and the untampered descriptor decodes)
    assert [st for st, _, _ in enc.decode_device_views_hwc(db)] == [0, 0]
    torch.cuda.synchronize()
    assert not bool((buf.view(torch.uint8) == SENTINEL).all())
