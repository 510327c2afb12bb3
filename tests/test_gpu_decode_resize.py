"""GPU decoder of a crop of each file RESIZED to a fixed size and optionally mirrored (-m gpu; fpng_amd_decode_batch_planar_resize /
fpng_amd_decode_batch_device_planar_resize: the crop kernels into the decode scratch, then dec_resize_kernel): uint8 planes and the
three float dtypes, three and four planes, mirror off and on, every pitch kind, host and device files.

Expected values never come from the library: the pixels are the REFERENCE's decoder's (judge()), sliced to the crop, resized by
resize_model.py (test_resize_cpu.py pins that text to Pillow), and for the float dtypes looked up in test_gpu_decode_float's table
(one fma in exact float64 arithmetic, rounded to the dtype).  Buffers are sentinel-filled and compared WHOLE and bit for bit, so not
one element outside the num_chans x out_h spans of out_w elements may change.

The kernel's tile is 64 columns x 16 rows of the OUTPUT: the sizes below hold 63 x 15, 64 x 16 and 65 x 17 (one below, at and one
past a tile in both axes), 224 x 224 (4 x 14 tiles), single rows and columns, and 1 x 1."""
import numpy as np
import pytest

from test_gpu_decode import UNDECIDED, _device_files, judge
from test_gpu_decode_float import CONSTS, _bits as _table_bits, _tables
from test_gpu_decode_layouts import SENTINEL, _damaged_files, _encode_gpu, _header_dims
from test_gpu_decode_planar import KINDS, _Region
import resize_model as RM

pytestmark = pytest.mark.gpu

DTYPES = ["uint8", "float32", "float16", "bfloat16"]
ELEM = {"uint8": 1, "float32": 4, "float16": 2, "bfloat16": 2}
BITS = {1: np.uint8, 2: np.uint16, 4: np.uint32}
CROP_OUTSIDE = 67
# (crop (x, y, w, h), size (out_w, out_h)) of the 600 x 130 files: shrink in x and grow in y; the identity across a tile border of
# the pixel pass; an upscale one past an output tile in both axes; a non-integer shrink; exactly 32 x; everything into one sample;
# one pixel into many; an inner tile of the pixel pass onto exactly one output tile and one short of it; a row; a column
CASES_600 = [((0, 0, 600, 130), (224, 224)), ((250, 40, 13, 20), (13, 20)), ((5, 7, 9, 11), (65, 17)), ((1, 1, 250, 100), (37, 19)),
             ((0, 0, 96, 64), (3, 2)), ((0, 0, 16, 16), (1, 1)), ((599, 129, 1, 1), (9, 9)), ((256, 48, 256, 48), (64, 16)),
             ((256, 48, 256, 48), (63, 15)), ((0, 77, 600, 1), (130, 1)), ((300, 0, 1, 130), (1, 33))]
CASES_OTHER = {(257, 49): [((0, 0, 257, 49), (9, 3)), ((1, 1, 255, 47), (64, 16)), ((256, 48, 1, 1), (2, 3)), ((3, 2, 100, 40), (100, 17))],
               (64, 97): [((0, 0, 64, 97), (33, 50)), ((7, 5, 50, 90), (128, 3))],
               (1, 1): [((0, 0, 1, 1), (5, 5)), ((0, 0, 1, 1), (1, 1))]}


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


class _Files:
    """the files, and the model's bytes of (file, crop, size), computed once each from the reference's decoder's four planes"""

    def __init__(self, pngs, dims, chans):
        self.pngs, self.dims, self.chans = pngs, dims, chans
        self.planes = []
        for p in pngs:
            st, px, w, h, _ = judge(p, 4)
            assert st == 0
            self.planes.append(np.ascontiguousarray(np.asarray(px)[: w * h * 4].reshape(h, w, 4).transpose(2, 0, 1)))
        self._resized = {}

    def resized(self, i, crop, size):
        """(4, out_h, out_w) uint8, not mirrored; read-only"""
        key = (i, crop, size)
        if key not in self._resized:
            x, y, w, h = crop
            r = RM.resize_planes(self.planes[i][:, y:y + h, x:x + w], size[0], size[1])
            r.setflags(write=False)
            self._resized[key] = r
        return self._resized[key]

    def cases(self):
        out = []
        for i, d in enumerate(self.dims):
            out += [(i, crop, size) for crop, size in (CASES_600 if d == (600, 130) else CASES_OTHER[d])]
        return out


@pytest.fixture(scope="module")
def files(enc):
    """600 x 130 and 257 x 49 in 3 and 4 channels, 1-pass, 2-pass and `noise` stored; 64 x 97 and 1 x 1 in two forms each"""
    import fpng_amd
    items, k = [], 0
    for (w, h) in ((600, 130), (257, 49)):
        for c in (3, 4):
            for fl in (0, 1, 2):
                items.append((fpng_amd.synth_image(("grad", "blocks")[k % 2] if fl != 2 else "noise", w, h, c, seed=k), fl))
                k += 1
    for (w, h), c, fl in (((64, 97), 3, 0), ((64, 97), 4, 2), ((1, 1), 3, 1), ((1, 1), 4, 0)):
        items.append((fpng_amd.synth_image("noise" if fl == 2 else "blocks", w, h, c, seed=k), fl))
        k += 1
    pngs = [bytes(p) for p in _encode_gpu(enc, items)]
    return _Files(pngs, [(im.shape[1], im.shape[0]) for im, _ in items], [im.shape[2] for im, _ in items])


def _regions(sizes, c, kinds):
    regs, off = [], 0
    for (ow, oh), kind in zip(sizes, kinds):
        r = _Region(off, ow, oh, c, kind)
        regs.append(r)
        off += r.size
    return regs, off


def _decode_resize(enc, pngs, crops, regs, total, dtype, device, mirror, consts=CONSTS[0], dev=None):
    """one call into ONE sentinel-filled buffer of `total` elements: (results, the elements' bits afterwards, the views)"""
    import torch
    e = ELEM[dtype]
    buf = torch.full((total * e,), SENTINEL, dtype=torch.uint8, device="cuda")
    typed = buf.view(getattr(torch, dtype))
    views = [typed.as_strided((r.c, r.h, r.w), (r.pp, r.rp, 1), r.lo) for r in regs]
    orders, ups = [r.order() for r in regs], [r.kind == "bottom_up" for r in regs]
    kw = {} if dtype == "uint8" else {"scale": consts[0], "bias": consts[1]}
    if device:
        got = enc.decode_device_resize(dev if dev is not None else _device_files(pngs, shift=1), crops, views, mirror=mirror, order=orders, bottom_up=ups, **kw)
    else:
        got = enc.decode_batch_resize(pngs, crops, views, mirror=mirror, order=orders, bottom_up=ups, **kw)
    torch.cuda.synchronize()
    return got, buf.cpu().numpy().view(BITS[e]), views


def _elements(r4, c, dtype, mirror, consts=CONSTS[0]):
    """(4, oh, ow) model bytes -> the (oh, ow, c) element bits a destination of c planes must hold"""
    px = r4[:c, :, ::-1] if mirror else r4[:c]
    px = np.ascontiguousarray(px.transpose(1, 2, 0))
    return px if dtype == "uint8" else _table_bits(px, _tables(consts, dtype))


def _expect(total, dtype, regs, sources):
    """the buffer a call must leave: the sentinel, and in every region whose source is not None its (oh, ow, c) elements"""
    exp = np.full(total, _sentinel(dtype), dtype=BITS[ELEM[dtype]])
    for r, src in zip(regs, sources):
        if src is not None:
            r.put(exp, src)
    return exp


def _first_difference(host, exp, regs):
    bad = np.nonzero(host != exp)[0]
    if not bad.size:
        return None
    return (bad.size, int(bad[0]), hex(int(host[bad[0]])), hex(int(exp[bad[0]])), [(i, r.w, r.h, r.kind, int(bad[0]) - r.lo) for i, r in enumerate(regs) if r.off <= bad[0] < r.off + r.size])


def _run_cases(enc, files, cases, c, dtype, device, mirrors, kinds):
    crops, sizes = [crop for _, crop, _ in cases], [size for _, _, size in cases]
    regs, total = _regions(sizes, c, kinds)
    got, host, views = _decode_resize(enc, [files.pngs[i] for i, _, _ in cases], crops, regs, total, dtype, device, mirrors)
    for k, ((i, _, _), (st, view, cf)) in enumerate(zip(cases, got)):
        assert st == 0 and cf == files.chans[i] and view is views[k], (k, i, st, cf)
    exp = _expect(total, dtype, regs, [_elements(files.resized(i, crop, size), c, dtype, m) for (i, crop, size), m in zip(cases, mirrors)])
    diff = _first_difference(host, exp, regs)
    assert diff is None, (c, dtype, device, diff, [cases[j] for j, *_ in diff[4]])


@pytest.mark.parametrize("mirror", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", [3, 4])
def test_resize_matrix_device_files(enc, files, c, dtype, mirror):
    """every file x every case of its size, into three and four planes of every dtype, mirror off and on, pitch kinds dealt
    round-robin: ONE call into ONE buffer that is compared whole"""
    cases = files.cases()
    kinds = [KINDS[(k + c) % len(KINDS)] for k in range(len(cases))]
    _run_cases(enc, files, cases, c, dtype, True, [mirror] * len(cases), kinds)


@pytest.mark.parametrize("c,dtype,mirror", [(3, "uint8", True), (4, "bfloat16", False), (4, "float32", True)])
def test_resize_matrix_host_files(enc, files, c, dtype, mirror):
    """the same through fpng_amd_decode_batch_planar_resize (files in host memory), for a subset"""
    cases = files.cases()[::2]
    kinds = [KINDS[(k + 2 * c) % len(KINDS)] for k in range(len(cases))]
    _run_cases(enc, files, cases, c, dtype, False, [mirror] * len(cases), kinds)


@pytest.mark.parametrize("kind", KINDS)
def test_every_pitch_kind(enc, files, kind):
    """tight, odd and padded pitches, bottom-up rows and planes in reverse order ("bgr" / "abgr"), f16: every case of one 3-channel
    and one 4-channel 600 x 130 file with that ONE kind, mirror flags alternating; the constants belong to the FILE's channels"""
    cases = [(i, crop, size) for i in (1, 3) for crop, size in CASES_600]
    assert files.dims[1] == files.dims[3] == (600, 130) and (files.chans[1], files.chans[3]) == (3, 4)
    for c in (3, 4):
        _run_cases(enc, files, cases, c, "float16", True, [bool(k & 1) for k in range(len(cases))], [kind] * len(cases))


def _mixed(files):
    """a batch of ten: different files, crops, sizes and mirror flags, stored and compressed; file 4's crop leaves the image"""
    rng = np.random.default_rng(31)
    all_cases = files.cases()
    pick = [all_cases[int(v)] for v in rng.permutation(len(all_cases))[:10]]
    assert any(files.dims[i] != (600, 130) for i, _, _ in pick)
    i4 = pick[4][0]
    pick[4] = (i4, (files.dims[i4][0] - 1, 0, 2, 1), (7, 5))
    return pick, [bool(v) for v in rng.integers(0, 2, 10)]


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("dtype", ["uint8", "float16"])
def test_one_mixed_batch(enc, files, dtype, device):
    """Ten clean files and one damaged one in ONE call.  The file whose crop leaves the image gets status 67 with the file's w and h
    and its region stays untouched; the damaged file gets the status the CROP call gives it for the same crop, and nothing outside
    its spans is written; every other file is exact."""
    pick, mirrors = _mixed(files)
    damaged = None
    for p in _damaged_files():
        w, h = _header_dims(p)
        if not (1 <= w <= 600 and 1 <= h <= 600):
            continue
        crop = (0, max(h - 2, 0), w, min(h, 2))
        (st, _, _), = enc.decode_batch_crop([p], [crop])
        if st not in (0, UNDECIDED):
            damaged = (p, crop, (max(w // 3, 1), 3), st)
            break
    assert damaged is not None
    pngs = [files.pngs[i] for i, _, _ in pick] + [damaged[0]]
    crops = [crop for _, crop, _ in pick] + [damaged[1]]
    sizes = [size for _, _, size in pick] + [damaged[2]]
    mirrors = mirrors + [True]
    c = 3
    kinds = [KINDS[k % len(KINDS)] for k in range(len(pngs))]
    regs, total = _regions(sizes, c, kinds)
    got, host, _ = _decode_resize(enc, pngs, crops, regs, total, dtype, device, mirrors)
    sts = [st for st, _, _ in got]
    assert sts == [0] * 4 + [CROP_OUTSIDE] + [0] * 5 + [damaged[3]], sts
    sources = [None if k == 4 else _elements(files.resized(i, crop, size), c, dtype, mirrors[k]) for k, (i, crop, size) in enumerate(pick)] + [None]
    exp = _expect(total, dtype, regs, sources)
    for a, b in regs[10].spans():  # (what a rejected file's spans hold is not defined)
        exp[a:b] = host[a:b]
    assert _first_difference(host, exp, regs) is None, _first_difference(host, exp, regs)


def test_results_report_the_files_dimensions_and_bad_records_launch_nothing(enc, files):
    import torch
    import fpng_amd
    n = len(files.pngs)
    batch = torch.full((n, 3, 4, 6), SENTINEL, dtype=torch.uint8, device="cuda")
    db = enc.decode_device_resize(_device_files(files.pngs), [(0, 0, 1, 1)] * n, list(batch), results=False)
    assert [(r.w, r.h, r.channels_in_file, r.status) for r in db.res] == [(w, h, c, 0) for (w, h), c in zip(files.dims, files.chans)]
    torch.cuda.synchronize()
    want = torch.from_numpy(np.stack([files.planes[i][:3, :1, :1] for i in range(n)])).cuda().expand(n, 3, 4, 6)
    assert torch.equal(batch, want)  # (one pixel into many: that pixel)
    # a bad record anywhere is the CALL's error: the valid files in front of it are not written either
    for field, value in (("reserved", 1), ("flags", 2), ("out_w", 0)):
        batch.fill_(SENTINEL)
        db = enc.make_decode_batch_resize(_device_files(files.pngs), [(0, 0, 1, 1)] * n, list(batch))
        setattr(db.sizes[n - 1], field, value)
        with pytest.raises(fpng_amd.FpngAmdError) as e:
            enc.decode_device_resize(db)
        torch.cuda.synchronize()
        assert e.value.code == -1 and bool((batch == SENTINEL).all()), field
    db = enc.make_decode_batch_resize(_device_files(files.pngs[:1]), [(0, 0, 192, 100)], [batch[0, :, :4, :6]])
    db.crops[0].w = 6 * 32 + 1  # (192 x 100 -> 6 x 4 is inside the limit)
    with pytest.raises(fpng_amd.FpngAmdError):
        enc.decode_device_resize(db)
    with pytest.raises(ValueError):
        enc.decode_batch_resize(db)  # (device files: decode_device_resize)
    with pytest.raises(ValueError):
        enc.decode_device_crop(db)


@pytest.mark.parametrize("device", [False, True])
def test_checksums_verified(enc, files, device):
    """set_decode_verify(CRC-32 and Adler-32): every tile of every file runs under the Adler-32 check; the outputs are the same and
    the statuses are the crop call's under the same flags"""
    import fpng_amd
    cases = files.cases()[1::3]
    crops = [crop for _, crop, _ in cases]
    pngs = [files.pngs[i] for i, _, _ in cases]
    kinds = [KINDS[k % len(KINDS)] for k in range(len(cases))]
    try:
        enc.set_decode_verify(fpng_amd.VERIFY_CRC32 | fpng_amd.VERIFY_ADLER32)
        want = [st for st, _, _ in (enc.decode_device_crop(_device_files(pngs), crops) if device else enc.decode_batch_crop(pngs, crops))]
        assert want == [0] * len(cases)
        _run_cases(enc, files, cases, 4, "bfloat16", device, [bool(k & 1) for k in range(len(cases))], kinds)
    finally:
        enc.set_decode_verify(0)


def test_a_descriptor_decodes_again_after_its_outputs_are_overwritten(enc, files):
    import torch
    cases = files.cases()[::4]
    dev = _device_files([files.pngs[i] for i, _, _ in cases], shift=2)
    for dtype in ("uint8", "float32"):
        outs = [torch.zeros((3 + (k & 1), oh, ow), dtype=getattr(torch, dtype), device="cuda") for k, (_, _, (ow, oh)) in enumerate(cases)]
        kw = {} if dtype == "uint8" else {"scale": CONSTS[0][0], "bias": CONSTS[0][1]}
        db = enc.make_decode_batch_resize(dev, [crop for _, crop, _ in cases], outs, mirror=[bool(k & 2) for k in range(len(cases))], **kw)
        for again in range(2):
            for t in outs:
                t.fill_(1)
            assert enc.decode_device_resize(db, results=False) is db
            torch.cuda.synchronize()
            assert list(db.statuses()) == [0] * len(cases)
            for k, ((i, crop, size), t) in enumerate(zip(cases, outs)):
                bits = t.cpu().view(torch.uint8).numpy().view(BITS[ELEM[dtype]])
                want = _elements(files.resized(i, crop, size), 3 + (k & 1), dtype, bool(k & 2)).transpose(2, 0, 1)
                assert np.array_equal(bits, want), (dtype, again, k)


def test_loader_batch_with_mean_and_std(enc, files):
    """an (n, 3, 32, 32) f16 batch filled in place through list(batch) with ImageNet's mean / std, mirror flags per file: within the
    bound test_gpu_decode_float holds for normalize_constants (the constants' and the fp32 result's rounding, 9.4 * 2^-24 < 6e-7,
    plus half an f16 ulp of the result, 2^-11 relative) of (byte / 255 - mean) / std in float64 on the MODEL's bytes; size= allocates"""
    import torch
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    idx = [0, 4, 7, 12]
    rng = np.random.default_rng(99)
    crops = []
    for i in idx:
        w, h = files.dims[i]
        cw, ch = int(rng.integers(8, min(w, 400) + 1)), int(rng.integers(8, h + 1))
        crops.append((int(rng.integers(0, w - cw + 1)), int(rng.integers(0, h - ch + 1)), cw, ch))
    mirrors = [False, True, True, False]
    dev = _device_files([files.pngs[i] for i in idx])
    batch = torch.full((4, 3, 32, 32), float("nan"), dtype=torch.float16, device="cuda")
    got = enc.decode_device_resize(dev, crops, list(batch), mirror=mirrors, mean=mean, std=std)
    torch.cuda.synchronize()
    m64, s64 = np.asarray(mean)[:, None, None], np.asarray(std)[:, None, None]
    for k, ((st, v, cf), i, crop) in enumerate(zip(got, idx, crops)):
        assert st == 0 and cf == files.chans[i] and v.data_ptr() == batch[k].data_ptr()
        r = files.resized(i, crop, (32, 32))[:3]
        ref = ((r[:, :, ::-1] if mirrors[k] else r).astype(np.float64) / 255.0 - m64) / s64
        out = batch[k].cpu().double().numpy()
        assert bool((np.abs(out - ref) <= 6e-7 + 2.0 ** -11 * np.abs(ref)).all()), (k, float(np.abs(out - ref).max()))
    got2 = enc.decode_device_resize(dev, crops, size=(32, 32), mirror=mirrors, dtype=torch.float16, mean=mean, std=std)
    assert all(st == 0 and v.dtype == torch.float16 and torch.equal(v.view(torch.int16), batch[k].view(torch.int16)) for k, (st, v, _) in enumerate(got2))
    got3 = enc.decode_device_resize(dev, crops, size=(20, 24))  # (out_h, out_w): the crops are at most 400 x 130, inside 32 x
    assert all(st == 0 and v.dtype == torch.uint8 and tuple(v.shape) == (3, 20, 24) for st, v, _ in got3)
