"""GPU decoder of a CROP of each file into planar images (-m gpu; fpng_amd_decode_batch_planar_crop /
fpng_amd_decode_batch_device_planar_crop, dec_unfilter_crop_kernel and dec_stored_crop_kernel): uint8 planes and the three float
dtypes, three and four planes, every pitch kind, host and device files.

Expected values are the FULL calls' (decode_device_planar, decode_device_float: other tests pin those to the reference's decoder and
to a single fused multiply-add), sliced -- and, for uint8, the reference's decoder's (judge()) directly.  Everything is compared
bit for bit: an element of a crop is the same byte, or the same fmaf and rounding, as the full call's.  Buffers are sentinel-filled
and compared WHOLE, so not one element outside the num_chans x crop.h spans of crop.w elements may change.
(test_hard_constants_at_cut_quads is the exception: its float values come from the table of test_gpu_decode_float, not from the
full call, at constants where the results tie, go subnormal or overflow.)"""
import ctypes as C
import os

import numpy as np
import pytest

from test_gpu_decode import UNDECIDED, _device_files, judge
from test_gpu_decode_float import CONSTS, HARD, _bits as _table_bits, _tables, hard_files
from test_gpu_decode_layouts import SENTINEL, _damaged_files, _encode_gpu, _header_dims
from test_gpu_decode_planar import KINDS, _Region
import verify_files as vf

pytestmark = pytest.mark.gpu

DTYPES = ["uint8", "float32", "float16", "bfloat16"]
ELEM = {"uint8": 1, "float32": 4, "float16": 2, "bfloat16": 2}
BITS = {1: np.uint8, 2: np.uint16, 4: np.uint32}
CROP_OUTSIDE, NOT_FPNG = 67, 1  # (FPNG_AMD_DECODE_CROP_OUTSIDE, fpng::FPNG_DECODE_NOT_FPNG)
SIZES = [(600, 130), (257, 49), (200, 30), (1, 1), (64, 97)]  # tiles are 48 rows x 256 pixels: 3 x 3 ragged ones, 2 x 2, one, ...
# crops of the 600 x 130 files: the whole image; small; across a block and a segment border; exactly one inner tile; the last block
# and segment only; across a wave's 64-pixel border; the corners; quads cut at the front (widths 1, 2, 3, 5 at x = 1, 2, 3); a
# full-width row; a full-height column
CROPS_600 = ([(0, 0, 600, 130), (5, 7, 9, 11), (250, 40, 13, 20), (256, 48, 256, 48), (257, 96, 343, 34), (61, 0, 7, 1), (599, 129, 1, 1), (0, 0, 1, 1)]
             + [(x, 46 + x, w, 3) for x in (1, 2, 3) for w in (1, 2, 3, 5)] + [(0, 77, 600, 1), (300, 0, 1, 130)])


def _sentinel(dtype):
    return BITS[ELEM[dtype]](int.from_bytes(bytes([SENTINEL]) * ELEM[dtype], "little"))


@pytest.fixture(scope="module")
def enc(built_lib):
    import torch
    import fpng_amd
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    e = fpng_amd.Encoder(device=0)
    yield e
    e.close()


def _full(enc, pngs, c, dtype, dims, consts=CONSTS[0]):
    """the full calls on device files: per file the (c, h, w) array of element BITS, or None where the status is not 0; the statuses"""
    import torch
    tdt = getattr(torch, dtype)
    outs = [torch.zeros((c, max(h, 1), max(w, 1)), dtype=tdt, device="cuda") for w, h in dims]
    dev = _device_files(pngs, shift=1)
    if dtype == "uint8":
        got = enc.decode_device_planar(dev, outs)
    else:
        got = enc.decode_device_float(dev, outs, scale=consts[0], bias=consts[1])
    torch.cuda.synchronize()
    return [t.cpu().view(torch.uint8).numpy().view(BITS[ELEM[dtype]]) if st == 0 else None for (st, _, _), t in zip(got, outs)], [st for st, _, _ in got]


@pytest.fixture(scope="module")
def files(enc):
    """(pngs, dims, file channels, full[(c, dtype)][i]): every size in 3 and 4 channels, 1-pass and 2-pass, and `noise` stored; the
    full calls' output of every file, computed once; the uint8 ones are the reference's decoder's"""
    import fpng_amd
    items, k = [], 0
    for (w, h) in SIZES:
        for c in (3, 4):
            for fl in (0, 1, 2):
                kind = ("grad", "blocks")[k % 2] if fl != 2 else "noise"
                items.append((fpng_amd.synth_image(kind, w, h, c, seed=k), fl))
                k += 1
    pngs = [bytes(p) for p in _encode_gpu(enc, items)]
    dims = [(im.shape[1], im.shape[0]) for im, _ in items]
    full = {}
    for c in (3, 4):
        for dtype in DTYPES:
            full[(c, dtype)], sts = _full(enc, pngs, c, dtype, dims)
            assert sts == [0] * len(pngs)
        for i, p in enumerate(pngs):
            cst, cpx, w, h, _ = judge(p, c)
            assert cst == 0 and np.array_equal(full[(c, "uint8")][i], np.asarray(cpx)[: w * h * c].reshape(h, w, c).transpose(2, 0, 1)), (i, c)
    return pngs, dims, [im.shape[2] for im, _ in items], full


def _regions(crops, c, kinds):
    regs, off = [], 0
    for (_, _, w, h), kind in zip(crops, kinds):
        r = _Region(off, w, h, c, kind)
        regs.append(r)
        off += r.size
    return regs, off


def _decode_crop(enc, pngs, crops, regs, total, dtype, device, consts=CONSTS[0], dev=None):
    """one call into ONE sentinel-filled buffer of `total` elements: (results, the elements' bits afterwards, the views)"""
    import torch
    e = ELEM[dtype]
    buf = torch.full((total * e,), SENTINEL, dtype=torch.uint8, device="cuda")
    typed = buf.view(getattr(torch, dtype))
    views = [typed.as_strided((r.c, r.h, r.w), (r.pp, r.rp, 1), r.lo) for r in regs]
    orders, ups = [r.order() for r in regs], [r.kind == "bottom_up" for r in regs]
    kw = {} if dtype == "uint8" else {"scale": consts[0], "bias": consts[1]}
    if device:
        got = enc.decode_device_crop(dev if dev is not None else _device_files(pngs, shift=1), crops, views, order=orders, bottom_up=ups, **kw)
    else:
        got = enc.decode_batch_crop(pngs, crops, views, order=orders, bottom_up=ups, **kw)
    torch.cuda.synchronize()
    return got, buf.cpu().numpy().view(BITS[e]), views


def _expect(total, dtype, regs, crops, sources):
    """the buffer a call must leave: the sentinel, and in every region whose source is not None its (c, h, w) array's window"""
    exp = np.full(total, _sentinel(dtype), dtype=BITS[ELEM[dtype]])
    for r, (x, y, w, h), src in zip(regs, crops, sources):
        if src is not None:
            r.put(exp, src[:, y:y + h, x:x + w].transpose(1, 2, 0))
    return exp


def _first_difference(host, exp, regs):
    bad = np.nonzero(host != exp)[0]
    if not bad.size:
        return None
    return (bad.size, int(bad[0]), hex(int(host[bad[0]])), hex(int(exp[bad[0]])), [(i, r.w, r.h, r.kind, int(bad[0]) - r.lo) for i, r in enumerate(regs) if r.off <= bad[0] < r.off + r.size])


def _other_crops(w, h, rng):
    """crops of the smaller files: the whole image, its last pixel, and a few seeded ones"""
    out = [(0, 0, w, h), (w - 1, h - 1, 1, 1)]
    for _ in range(3):
        cw, ch = int(rng.integers(1, w + 1)), int(rng.integers(1, h + 1))
        out.append((int(rng.integers(0, w - cw + 1)), int(rng.integers(0, h - ch + 1)), cw, ch))
    return out


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", [3, 4])
def test_crop_matrix(enc, files, c, dtype, device):
    """3- and 4-channel files x 1-pass, 2-pass and stored x every crop of CROPS_600 (and a few crops of every other size) x pitch kinds
    dealt round-robin, into three and four planes of every dtype through both entry points: ONE call per case into ONE buffer that
    is compared whole -- the full call's elements in every span, the sentinel everywhere else; results carry the FILE's dimensions."""
    pngs, dims, chans, full = files
    rng = np.random.default_rng(17)
    batch = []
    for i, (w, h) in enumerate(dims):
        for crop in (CROPS_600 if (w, h) == (600, 130) else _other_crops(w, h, rng)):
            batch.append((i, crop))
    kinds = [KINDS[k % len(KINDS)] for k in range(len(batch))]
    crops = [crop for _, crop in batch]
    regs, total = _regions(crops, c, kinds)
    got, host, views = _decode_crop(enc, [pngs[i] for i, _ in batch], crops, regs, total, dtype, device)
    for k, ((i, _), (st, view, cf)) in enumerate(zip(batch, got)):
        assert st == 0 and cf == chans[i] and view is views[k], (k, i, st, cf)
    exp = _expect(total, dtype, regs, crops, [full[(c, dtype)][i] for i, _ in batch])
    assert _first_difference(host, exp, regs) is None, (c, dtype, device, _first_difference(host, exp, regs))


@pytest.mark.parametrize("dtype", DTYPES[1:])
@pytest.mark.parametrize("name", sorted(HARD))
def test_hard_constants_at_cut_quads(enc, name, dtype):
    """test_gpu_decode_float's hard constant sets and files (w = 257 ... 260, every byte value at every quad position) through the
    crop kernels: crops that cut the first quad by 1, 2 and 3 elements and the last quad as well, and the whole image, into three
    and four planes.  The expected bits are the TABLE's (one fma in exact float64 arithmetic, round to nearest even) at the
    reference's pixels -- not the full call's, so that a mistake the two kernels share cannot cancel."""
    pngs, judged = hard_files()
    tab = _tables(HARD[name], dtype)
    k = sorted(HARD).index(name) + DTYPES.index(dtype)
    for c in (3, 4):
        batch, sources = [], []
        for i, p in enumerate(pngs):
            st, px, w, h, _ = judged[c][i]
            src = _table_bits(np.asarray(px)[: w * h * c].reshape(h, w, c), tab).transpose(2, 0, 1)
            for crop in ((1, 0, w - 1, 256), (2, 1, w - 3, 255), (3, 0, w - 3, 256), (0, 0, w, 256)):
                batch.append((i, crop))
                sources.append(src)
        crops = [crop for _, crop in batch]
        kinds = [KINDS[(j + k + c) % len(KINDS)] for j in range(len(batch))]
        regs, total = _regions(crops, c, kinds)
        device = bool((k + c) & 1)
        got, host, views = _decode_crop(enc, [pngs[i] for i, _ in batch], crops, regs, total, dtype, device, consts=HARD[name])
        assert [st for st, _, _ in got] == [0] * len(batch)
        exp = _expect(total, dtype, regs, crops, sources)
        assert _first_difference(host, exp, regs) is None, (name, c, dtype, device, _first_difference(host, exp, regs))


def test_results_report_the_files_dimensions(enc, files):
    pngs, dims, chans, _ = files
    import torch
    crops = [(0, 0, 1, 1)] * len(pngs)
    outs = [torch.zeros((3, 1, 1), dtype=torch.uint8, device="cuda") for _ in pngs]
    db = enc.decode_device_crop(_device_files(pngs), crops, outs, results=False)
    assert [(r.w, r.h, r.channels_in_file, r.status) for r in db.res] == [(w, h, c, 0) for (w, h), c in zip(dims, chans)]


def test_one_mixed_batch_next_to_plain_calls(enc, files):
    """16 files of different sizes, crops, channel counts, stored and compressed, in ONE call; the same descriptor again after the
    outputs were overwritten; plain planar and float calls on the same encoder before and after give what they gave."""
    import torch
    pngs, dims, chans, full = files
    rng = np.random.default_rng(23)
    pick = [int(v) for v in rng.permutation(len(pngs))[:16]]
    sub, sdims = [pngs[i] for i in pick], [dims[i] for i in pick]
    crops = []
    for (w, h) in sdims:
        cw, ch = int(rng.integers(1, w + 1)), int(rng.integers(1, h + 1))
        crops.append((int(rng.integers(0, w - cw + 1)), int(rng.integers(0, h - ch + 1)), cw, ch))
    for dtype in ("uint8", "bfloat16"):
        before = _full(enc, sub, 4, dtype, sdims)
        tdt = getattr(torch, dtype)
        outs = [torch.zeros((3 + (k & 1), ch, cw), dtype=tdt, device="cuda") for k, (_, _, cw, ch) in enumerate(crops)]
        kw = {} if dtype == "uint8" else {"scale": CONSTS[0][0], "bias": CONSTS[0][1]}
        db = enc.make_decode_batch_crop(_device_files(sub, shift=2), crops, outs, **kw)
        for again in range(2):
            for t in outs:
                t.fill_(1)
            assert enc.decode_device_crop(db, results=False) is db
            torch.cuda.synchronize()
            assert list(db.statuses()) == [0] * 16
            for k, (i, (x, y, w, h), t) in enumerate(zip(pick, crops, outs)):
                c = 3 + (k & 1)
                bits = t.cpu().view(torch.uint8).numpy().view(BITS[ELEM[dtype]])
                assert np.array_equal(bits, full[(c, dtype)][i][:, y:y + h, x:x + w]), (dtype, again, k, i, (x, y, w, h))
        after = _full(enc, sub, 4, dtype, sdims)
        assert before[1] == after[1] == [0] * 16 and all(np.array_equal(a, b) for a, b in zip(before[0], after[0]))
    with pytest.raises(ValueError):
        enc.decode_batch_crop(db)  # (device files: decode_device_crop)
    with pytest.raises(ValueError):
        enc.decode_device_planar(db)


def _raw_call(enc, pngs, recs, crops, fmt, device):
    """the C entry points on hand-made records (num_chans, d_pixels, row_pitch, plane_pitch, cap), crops (x, y, w, h) and format
    (dtype, reserved, scale[4], bias[4]) or None: (rc, [(status, w, h)])"""
    import torch
    from fpng_amd import _lib
    n = len(recs)
    arr, carr, res = (_lib.PngPlanarIn * n)(), (_lib.Crop * n)(), (_lib.DecodeResult * n)()
    f = None
    if fmt is not None:
        f = _lib.FloatFormat()
        f.dtype, f.reserved = fmt[0], fmt[1]
        for k in range(4):
            f.scale[k], f.bias[k] = fmt[2][k], fmt[3][k]
    keep = _device_files(pngs, shift=1) if device else [np.frombuffer(bytes(p), dtype=np.uint8) for p in pngs]
    for i, (c, ptr, rp, pp, cap) in enumerate(recs):
        arr[i].data = keep[i].data_ptr() if device else keep[i].ctypes.data
        arr[i].size = len(pngs[i])
        arr[i].num_chans, arr[i].d_pixels, arr[i].row_pitch, arr[i].plane_pitch, arr[i].pixels_cap = c, ptr, rp, pp, cap
        carr[i].x, carr[i].y, carr[i].w, carr[i].h = crops[i]
    fn = enc.lib.fpng_amd_decode_batch_device_planar_crop if device else enc.lib.fpng_amd_decode_batch_planar_crop
    enc._sync_stream()
    rc = fn(enc.h, arr, carr, n, C.byref(f) if f is not None else None, res)
    torch.cuda.synchronize()
    return rc, [(r.status, r.w, r.h) for r in res]


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("dtype", ["uint8", "float16"])
def test_a_crop_that_leaves_the_image_is_its_files_outcome(enc, files, dtype, device):
    """Files 1 and 3 of a batch of five: a crop one pixel past the right edge (x = 0xFFFFFFFF, w = 2: the sum needs 64 bits) and one
    past the bottom edge -- status 67 with the file's w and h, no room needed and nothing written for them; the others exact."""
    import torch
    pngs, dims, chans, full = files
    idx = [0, 1, 6, 9, 13]
    assert dims[1] == (600, 130) and dims[9][1] == 49
    crops = [(5, 7, 9, 11), (0xFFFFFFFF, 0, 2, 1), (3, 3, 40, 20), (10, dims[9][1] - 4, 6, 5), (0, 0, 7, 5)]
    e = ELEM[dtype]
    fmt = None if dtype == "uint8" else (DTYPES.index(dtype) - 1, 0, [float(v) for v in CONSTS[0][0]], [float(v) for v in CONSTS[0][1]])
    buf = torch.full((1 << 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    base, slot = buf.data_ptr(), 1 << 13
    recs = [(3, base + k * slot, 0, 0, 3 * w * h * e) for k, (_, _, w, h) in enumerate(crops)]
    recs[1], recs[3] = (3, 0, 0, 0, 0), (3, base + 3 * slot, 0, 0, 1)  # (no room is needed)
    rc, res = _raw_call(enc, [pngs[i] for i in idx], recs, crops, fmt, device)
    assert rc == 0, rc
    assert res == [(CROP_OUTSIDE if k in (1, 3) else 0,) + dims[i] for k, i in enumerate(idx)]
    host = buf.cpu().numpy().view(BITS[e])
    exp = np.full(host.size, _sentinel(dtype), dtype=host.dtype)
    for k, (i, (x, y, w, h)) in enumerate(zip(idx, crops)):
        if k not in (1, 3):
            exp[k * slot // e: k * slot // e + 3 * w * h] = full[(3, dtype)][i][:, y:y + h, x:x + w].reshape(-1)
    assert np.array_equal(host, exp)
    # an empty crop is the CALL's error, and nothing is launched: the valid file in front of it is not written either
    for bad in ((5, 7, 0, 11), (5, 7, 9, 0)):
        buf.fill_(SENTINEL)
        rc, _ = _raw_call(enc, [pngs[0], pngs[1]], [recs[0], recs[2]], [crops[0], bad], fmt, device)
        assert rc == -1 and bool((buf == SENTINEL).all()), bad


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_validation(enc, dtype, device):
    """The planar and float calls' rules with the CROP's dimensions in the place of the file's: every rule gets its error code, the
    call writes nothing (also not the valid file's part in front of the bad one), and the next valid call -- exact cap, odd element
    offset and pitches, negative pitches -- succeeds."""
    import torch
    INVALID, SMALL = -1, -4
    e = ELEM[dtype]
    fw, fh = 37, 21
    good = bytes(_encode_gpu(enc, [(np.random.default_rng(3).integers(0, 256, (fh, fw, 4), dtype=np.uint8), 0)])[0])
    crop = (3, 2, 29, 15)
    _, _, w, h = crop
    buf = torch.full((1 << 17,), SENTINEL, dtype=torch.uint8, device="cuda")
    base = buf.data_ptr()
    one, zero = [1.0 / 255.0] * 4, [0.0] * 4
    code = DTYPES.index(dtype) - 1
    fmt = None if dtype == "uint8" else (code, 0, one, zero)
    full = (3 * w * h + (h - 1) * w + w) * e  # span of four tight planes of the crop's size, in bytes
    ok = (4, base, 0, 0, full)
    far = base + 32768
    rp, pp = (w + 3) * e, (h * (w + 3) + 1) * e
    span3 = 2 * pp + (h - 1) * rp + w * e
    inf, nan = float("inf"), float("nan")
    cases = [
        ((4, far, (w - 1) * e, 0, 1 << 15), fmt, INVALID),                       # |row_pitch| < crop.w elements
        ((4, far + (h - 1) * w * e, -(w - 1) * e, h * w * e, 1 << 15), fmt, INVALID),
        ((4, far, w * e, (h * w - 1) * e, 1 << 15), fmt, INVALID),               # planes overlap
        ((3, far + 2 * h * w * e, w * e, -(h * w - 1) * e, 1 << 15), fmt, INVALID),
        ((3, far, (w + 8) * e, h * w * e, 1 << 15), fmt, INVALID),               # ... because of the rows' padding
        ((5, far, 0, 0, 1 << 15), fmt, INVALID),                                 # num_chans
        ((3, far, 1 << 31, 0, 1 << 15), fmt, INVALID),                           # |row_pitch| >= 2^31
        ((4, far, 0, 0, full - 1), fmt, SMALL),                                  # cap one byte short
        ((3, far + e, rp, pp, span3 - 1), fmt, SMALL),
        ((4, 0, 0, 0, 1 << 15), fmt, SMALL),                                     # no buffer
    ]
    if dtype != "uint8":
        cases += [
            ((4, far + e // 2, 0, 0, 1 << 15), fmt, INVALID),                    # a base that is no multiple of the element size
            ((4, far + 1, 0, 0, 1 << 15), fmt, INVALID),
            ((3, far, rp + 1, pp, 1 << 15), fmt, INVALID),                       # ... a row pitch
            ((3, far, rp, pp + e // 2, 1 << 15), fmt, INVALID),                  # ... a plane pitch
            (ok, (3, 0, one, zero), INVALID),                                    # dtype
            (ok, (code, 1, one, zero), INVALID),                                 # reserved
            (ok, (code, 0, [1.0, inf, 1.0, 1.0], zero), INVALID),                # a scale or bias that is not finite
            (ok, (code, 0, one, [0.0, 0.0, 0.0, nan]), INVALID),
        ]
    for rec, f, want in cases:
        rc, _ = _raw_call(enc, [good, good], [ok, rec], [crop, crop], f, device)
        assert rc == want, (rec, f, rc)
        assert bool((buf == SENTINEL).all()), (rec, f)
    # (a cap that would hold the crop but not the file is enough: the file's size does not count)
    assert full < 4 * fw * fh * e
    o3, o4 = 32768 + e, 65536
    rc, res = _raw_call(enc, [good, good, good], [ok, (3, base + o3, rp, pp, span3), (4, base + o4 + (3 * h * w + (h - 1) * w) * e, -w * e, -h * w * e, full)],
                        [crop] * 3, fmt, device)
    assert rc == 0 and res == [(0, fw, fh)] * 3, (rc, res)
    src, sts = _full(enc, [good], 4, dtype, [(fw, fh)], consts=(np.float32(one), np.float32(zero)))
    px = src[0][:, crop[1]:crop[1] + h, crop[0]:crop[0] + w]  # (4, h, w)
    host = buf.cpu().numpy().view(BITS[e])
    exp = np.full(host.size, _sentinel(dtype), dtype=host.dtype)
    exp[: 4 * h * w] = px.reshape(-1)
    for ch in range(3):
        for y in range(h):
            a = (o3 + ch * pp + y * rp) // e
            exp[a: a + w] = px[ch, y]
    exp[o4 // e: o4 // e + 4 * h * w] = px[::-1, ::-1].reshape(-1)  # planes A,B,G,R, rows bottom-up
    assert np.array_equal(host, exp)


# ---- the status rule: what the pixel pass finds, it finds only in the tiles that run ----
@pytest.fixture(scope="module")
def tall(enc):
    """600 x 300 RGB and RGBA files (7 segments x 3 column blocks) with their token streams opened for edits, and their full decodes"""
    import fpng_amd
    import test_decode_model as M
    import token_mutator as TM
    from test_gpu_decode_status import _encode
    out = {}
    for c, kind in ((3, "blocks"), (4, "grad")):
        img = fpng_amd.synth_image(kind, 600, 300, c, seed=c)
        png = bytes(_encode(np.ascontiguousarray(img).reshape(-1), 600, 300, c, 0))
        clean, sts = _full(enc, [png], 3, "uint8", [(600, 300)])
        assert sts == [0]
        out[c] = (png, TM.LargeStream(png, M.plan, M.emul()), clean[0])
    return out


def _one_crop(enc, png, crop, dtype="uint8", device=True, c=3):
    """a single file's crop into a sentinel-filled region: (status, bits of the whole buffer, region)"""
    regs, total = _regions([crop], c, ["odd"])
    got, host, _ = _decode_crop(enc, [png], [crop], regs, total, dtype, device)
    return got[0][0], host, regs, total


@pytest.mark.parametrize("kind", ["filter_byte", "lit2match_firstpx"])
@pytest.mark.parametrize("c", [3, 4])
def test_status_rule(enc, tall, c, kind):
    """One edit that only the pixel pass can find, in column block 0 (a filter byte that is not 2; a match at a row's first pixel):
    (a) below the crop's rows and (b) beside its columns the file decodes with 0 and the crop is the clean file's; (c) inside the
    needed tiles the status is the full call's -- NOT_FPNG, or UNDECIDED for the match."""
    from test_gpu_decode_status import _edited
    png, s, clean = tall[c]
    rng = np.random.default_rng(77 + c)
    want = NOT_FPNG if kind == "filter_byte" else UNDECIDED
    for rows, crops in (((200, 247), [((0, 0, 600, 100), 0)]), ((48, 95), [((300, 60, 200, 20), 0), ((0, 60, 200, 20), want)])):
        made = _edited(s, rng, kind, rows)
        assert made is not None, (kind, rows)
        f = bytes(made[0])
        _, full_st = _full(enc, [f], 3, "uint8", [(600, 300)])
        assert full_st == [want], (kind, rows, full_st)
        for crop, st_want in crops:
            for device in (False, True):
                st, host, regs, total = _one_crop(enc, f, crop, device=device)
                assert st == st_want, (kind, rows, crop, device, st)
                if st_want == 0:
                    assert np.array_equal(host, _expect(total, "uint8", regs, [crop], [clean])), (kind, rows, crop, device)
                else:  # (what a rejected file's spans hold is not defined; everything else is the sentinel)
                    assert np.array_equal(host, _expect(total, "uint8", regs, [crop], [None])) or _spans_only(host, regs), (kind, rows, crop)


def _spans_only(host, regs, dtype="uint8"):
    mask = np.ones(host.size, dtype=bool)
    for r in regs:
        for a, b in r.spans():
            mask[a:b] = False
    return bool(np.all(host[mask] == _sentinel(dtype)))


@pytest.mark.parametrize("device", [False, True])
def test_damaged_files_get_the_full_calls_status(enc, device):
    """container_mutator / token_mutator files with a small crop that touches every tile of the file (its last rows, full width):
    every status and channels_in_file is the full call's, also when every compressed file is UNDECIDED
    (FPNG_AMD_DECODE_MAX_ROUNDS=0), and nothing is written outside the spans."""
    pngs = _damaged_files()
    dims = [_header_dims(p) for p in pngs]
    crops = [(0, max(h - 2, 0), w, min(h, 2)) for w, h in dims]
    kinds = [KINDS[i % len(KINDS)] for i in range(len(pngs))]
    for k, (c, dtype) in enumerate(((3, "uint8"), (4, "float16"))):
        for forced in (False, True):
            if forced:
                os.environ["FPNG_AMD_DECODE_MAX_ROUNDS"] = "0"
            try:
                packed = enc.decode_batch(pngs, c)
                regs, total = _regions(crops, c, kinds)
                got, host, _ = _decode_crop(enc, pngs, crops, regs, total, dtype, device)
            finally:
                if forced:
                    del os.environ["FPNG_AMD_DECODE_MAX_ROUNDS"]
            sts = [st for st, _, _ in got]
            assert sts == [st for st, _, _ in packed], (c, forced)
            assert [cf for _, _, cf in got] == [cf for _, _, cf in packed], (c, forced)
            if forced:
                assert UNDECIDED in sts
            assert any(st not in (0, UNDECIDED) for st in sts)
            assert _spans_only(host, regs, dtype), (c, forced, device)


def test_checksums(enc, tall):
    """Both checks on, one literal changed in a row OUTSIDE the needed tiles: BAD_CRC32; with the CRC word repaired BAD_ADLER32 (every
    tile runs for the Adler-32); with only the CRC check on and the CRC repaired 0 and the clean file's crop.  A filter byte edited
    beside the crop's columns: with the Adler check on, the full call's status.  A clean file under both flags: 0 and exact crops."""
    from test_gpu_decode_status import _edited
    png, s, clean = tall[4]
    rng = np.random.default_rng(5)
    crop = (10, 20, 100, 50)  # segments 0 and 1 of column block 0
    made = vf.edit_literal_large(png, None, 250, 0, 600 * 4, rng, stream=s)
    assert made is not None
    crc_ok, crc_stale = made
    assert vf.adler_is_bad(crc_ok) and not vf.crc_is_bad(crc_ok) and vf.crc_is_bad(crc_stale)
    beside = _edited(s, np.random.default_rng(81), "filter_byte", (48, 95))
    assert beside is not None
    beside = bytes(beside[0])
    assert _one_crop(enc, beside, (300, 60, 200, 20))[0] == 0  # (without the check: the tile with the filter byte does not run)
    try:
        for device in (False, True):
            enc.set_decode_verify(3)
            assert _one_crop(enc, crc_stale, crop, device=device)[0] == 65
            assert _one_crop(enc, crc_ok, crop, device=device)[0] == 66
            for dtype in ("uint8", "float16"):
                st, host, regs, total = _one_crop(enc, png, crop, dtype=dtype, device=device)
                src, _ = _full(enc, [png], 3, dtype, [(600, 300)])
                assert st == 0 and np.array_equal(host, _expect(total, dtype, regs, [crop], [src[0]])), (dtype, device)
            enc.set_decode_verify(1)
            st, host, regs, total = _one_crop(enc, crc_ok, crop, device=device)
            assert st == 0 and np.array_equal(host, _expect(total, "uint8", regs, [crop], [clean])), device
            assert _one_crop(enc, crc_stale, crop, device=device)[0] == 65
            enc.set_decode_verify(2)
            _, full_st = _full(enc, [beside], 3, "uint8", [(600, 300)])
            st, host, regs, _ = _one_crop(enc, beside, (300, 60, 200, 20), device=device)
            assert full_st == [NOT_FPNG] and st == NOT_FPNG and _spans_only(host, regs), (device, st, full_st)
    finally:
        enc.set_decode_verify(0)


def test_random_crop_loader(enc):
    """decode_device_crop fills the views of one (n, 3, 224, 224) f16 batch in place from 512 x 512 files with seeded random crops:
    bit-equal to decode_device_float and a slice."""
    import torch
    import fpng_amd
    n = 4
    items = [(fpng_amd.synth_image(("grad", "blocks", "noise", "grad")[k], 512, 512, 3 + (k & 1), seed=40 + k), k % 2) for k in range(n)]
    dev = _device_files(_encode_gpu(enc, items))
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    whole = torch.zeros((n, 3, 512, 512), dtype=torch.float16, device="cuda")
    assert [st for st, _, _ in enc.decode_device_float(dev, list(whole), mean=mean, std=std)] == [0] * n
    rng = np.random.default_rng(1234)
    crops = [(int(rng.integers(0, 512 - 224 + 1)), int(rng.integers(0, 512 - 224 + 1)), 224, 224) for _ in range(n)]
    batch = torch.full((n, 3, 224, 224), float("nan"), dtype=torch.float16, device="cuda")
    got = enc.decode_device_crop(dev, crops, list(batch), mean=mean, std=std)
    for k, ((st, v, cf), (x, y, w, h)) in enumerate(zip(got, crops)):
        assert st == 0 and cf == 3 + (k & 1) and v.data_ptr() == batch[k].data_ptr()
        assert torch.equal(batch[k].view(torch.int16), whole[k, :, y:y + h, x:x + w].contiguous().view(torch.int16)), (k, x, y)
    # outs=None allocates (3, h, w) tensors of the dtype asked for
    got = enc.decode_device_crop(dev, crops, dtype=torch.float16, mean=mean, std=std)
    for k, (st, v, _) in enumerate(got):
        assert st == 0 and v.dtype == torch.float16 and torch.equal(v.view(torch.int16), batch[k].view(torch.int16)), k
    got = enc.decode_device_crop(dev, crops)
    assert all(st == 0 and v.dtype == torch.uint8 and tuple(v.shape) == (3, 224, 224) for st, v, _ in got)
