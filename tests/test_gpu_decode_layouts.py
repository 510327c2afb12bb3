"""GPU decoder into other pixel layouts (-m gpu; fpng_amd_decode_batch_ex / fpng_amd_decode_batch_device_ex, the *_ex forms of
dec_unfilter_kernel and dec_stored_kernel): every destination format, pitch and row order against the REFERENCE's decoder at
desired 3 or 4 reordered in numpy (X bytes 0xFF), statuses against the packed call, and not one byte written outside the rows."""
import os
import struct

import numpy as np
import pytest

from cpu_ref import fuzz_image
from test_gpu_decode import UNDECIDED, _device_files, judge

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
NAMES = ["RGB", "BGR", "RGBA", "BGRA", "ARGB", "ABGR", "RGBX", "BGRX", "XRGB", "XBGR"]
KINDS = ["packed", "odd", "pad256", "bottom_up"]


@pytest.fixture(scope="module")
def enc(built_lib):
    import torch
    import fpng_amd
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    e = fpng_amd.Encoder(device=0)
    yield e
    e.close()


def _nbytes(name):
    return 3 if name in ("RGB", "BGR") else 4


def _reorder(px, name):
    """(h, w, 3 or 4) pixels in R,G,B[,A] order -> the format's bytes (X = 0xFF)"""
    idx = {"R": 0, "G": 1, "B": 2, "A": 3}
    out = np.empty(px.shape[:2] + (len(name),), dtype=np.uint8)
    for k, ch in enumerate(name):
        out[..., k] = 0xFF if ch == "X" else px[..., idx[ch]]
    return out


class _Region:
    """a file's destination inside one sentinel-filled buffer: `front` bytes of margin, h rows `pitch` bytes apart, a margin behind"""

    def __init__(self, off, w, h, nb, kind):
        self.w, self.h, self.nb, self.kind = w, h, nb, kind
        odd = kind == "odd" and nb == 3
        self.pitch = w * nb + (256 if kind == "pad256" else (7 if odd else (12 if kind == "odd" else 0)))
        self.front = 64 + (1 if odd else 0)
        self.off = off  # the region's first byte (4-byte aligned)
        self.lo = off + self.front  # the lowest-addressed row's first byte
        self.size = (self.front + (h - 1) * self.pitch + w * nb + 64 + 3) & ~3

    def row_offset(self, y):  # where the file's row y lies
        return self.lo + ((self.h - 1 - y) if self.kind == "bottom_up" else y) * self.pitch

    def spans(self):
        return [(self.row_offset(y), self.row_offset(y) + self.w * self.nb) for y in range(self.h)]


def _regions(dims, name, kinds):
    regs, off = [], 0
    for (w, h), kind in zip(dims, kinds):
        r = _Region(off, max(w, 1), max(h, 1), _nbytes(name), kind)
        regs.append(r)
        off += r.size
    return regs, off


def _views(buf, regs):
    return [buf.as_strided((r.h, r.w, r.nb), (r.pitch, r.nb, 1), r.lo) for r in regs]


def _decode_ex(enc, pngs, name, regs, total, device):
    """one call into a sentinel-filled buffer: (results, the buffer's bytes afterwards, its bytes before)"""
    import torch
    buf = torch.full((total,), SENTINEL, dtype=torch.uint8, device="cuda")
    views = _views(buf, regs)
    ups = [r.kind == "bottom_up" for r in regs]
    if device:
        got = enc.decode_device_ex(_device_files(pngs, shift=1), views, name.lower(), ups)
    else:
        got = enc.decode_batch_ex(pngs, views, name.lower(), ups)
    torch.cuda.synchronize()
    return got, buf.cpu().numpy(), views


def _outside_untouched(host, regs):
    mask = np.ones(host.size, dtype=bool)
    for r in regs:
        for a, b in r.spans():
            mask[a:b] = False
    return bool(np.all(host[mask] == SENTINEL))


def _encode_gpu(enc, imgs_flags):
    import torch
    out = []
    for img, fl in imgs_flags:
        (png,), _ = enc.encode_tensors([torch.from_numpy(np.ascontiguousarray(img)).cuda()], fl)
        out.append(png)
    return out


def _matrix_files(enc):
    import fpng_amd
    sizes = [(w, h) for w in (1, 63, 64, 65, 255, 256, 257) for h in (1, 47, 48, 49, 97)] + [(7680, 1), (7680, 49), (7680, 97)]
    items, k = [], 0
    for (w, h) in sizes:
        for c in (3, 4):
            for fl in (0, 1, 2):  # 1-pass, 2-pass, stored
                kind = ("grad", "blocks", "noise")[k % 3] if fl != 2 else "noise"
                items.append((fpng_amd.synth_image(kind, w, h, c, seed=k), fl))
                k += 1
    return _encode_gpu(enc, items)


@pytest.fixture(scope="module")
def matrix(enc):
    pngs = _matrix_files(enc)
    judged = {d: [judge(p, d) for p in pngs] for d in (3, 4)}
    packed = {d: enc.decode_batch(pngs, d) for d in (3, 4)}
    return pngs, judged, packed


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_every_format_pitch_and_width(enc, matrix, name, device):
    """Every format x 3- and 4-channel files x 1-pass, 2-pass and stored files x widths around the epilogue's edges (1, 63, 64, 65,
    255, 256, 257, 7680) x heights around the 48-row segment x pitch kinds (packed, odd start and pitch, +256, bottom-up), one call
    per format and entry point: the reference's pixels reordered, the packed call's statuses, nothing outside the rows."""
    pngs, judged, packed = matrix
    d = _nbytes(name)
    dims = [struct.unpack(">II", bytes(p[16:24])) for p in pngs]
    kinds = [KINDS[i % 4] for i in range(len(pngs))]
    regs, total = _regions(dims, name, kinds)
    got, host, views = _decode_ex(enc, pngs, name, regs, total, device)
    exp = np.full(total, SENTINEL, dtype=np.uint8)
    for i, (png, r, (st, view, cf)) in enumerate(zip(pngs, regs, got)):
        cst, cpx, w, h, c = judged[d][i]
        pst, _, pcf = packed[d][i]
        assert st == cst == pst == 0 and cf == c == pcf, (i, st, cst, pst)
        assert view is views[i]
        px = _reorder(np.asarray(cpx)[: w * h * d].reshape(h, w, d), name)
        for y in range(h):
            exp[r.row_offset(y): r.row_offset(y) + w * d] = px[y].reshape(-1)
    bad = np.nonzero(host != exp)[0]
    assert bad.size == 0, (name, device, [(i, r.w, r.h, r.kind) for i, r in enumerate(regs) if r.off <= bad[0] < r.off + r.size])


def _damaged_files():
    from test_decode_model import edited_files
    from test_dropin_decode import edited_containers
    rng = np.random.default_rng(5)
    files = [f for _, f in edited_containers(rng, 30)] + [f for _, f in edited_files(rng, 15)]
    return files


@pytest.mark.parametrize("device", [False, True])
def test_damaged_and_undecided_files_write_nothing_outside_the_rows(enc, device):
    """container_mutator / token_mutator files, and every compressed file UNDECIDED (FPNG_AMD_DECODE_MAX_ROUNDS=0): each status is
    the packed call's at the same desired channels, and every byte outside the row spans keeps its sentinel."""
    pngs = _damaged_files()
    for name in ("BGR", "RGB", "BGRA", "XRGB"):
        d = _nbytes(name)
        for forced in (False, True):
            if forced:
                os.environ["FPNG_AMD_DECODE_MAX_ROUNDS"] = "0"
            try:
                packed = enc.decode_batch(pngs, d)
                dims = [_header_dims(p) for p in pngs]
                kinds = [KINDS[i % 4] for i in range(len(pngs))]
                regs, total = _regions(dims, name, kinds)
                got, host, _ = _decode_ex(enc, pngs, name, regs, total, device)
            finally:
                if forced:
                    del os.environ["FPNG_AMD_DECODE_MAX_ROUNDS"]
            sts = [st for st, _, _ in got]
            assert sts == [st for st, _, _ in packed], (name, forced)
            assert [cf for _, _, cf in got] == [cf for _, _, cf in packed], (name, forced)
            if forced:
                assert UNDECIDED in sts
            assert any(st not in (0, UNDECIDED) for st in sts)
            assert _outside_untouched(host, regs), (name, forced, device)


def _header_dims(png):
    """room for a file: the dimensions the container walk reports (a damaged or undecided file's header may be accepted: it then
    needs its rows' room) when they are small, else one pixel (a file the walk rejects needs none)"""
    import ctypes as C
    from fpng_amd import _lib
    lib = _lib.load()
    r = _lib.DecodeResult()
    u32, u64, lut = C.c_uint32, C.c_uint64, (C.c_uint32 * 4160)()
    a, b, c, d, e = u32(), u32(), u32(), u64(), u64()
    b_ = bytes(png)
    lib.fpng_amd_decode_plan(b_, len(b_), C.byref(r), C.byref(a), C.byref(b), C.byref(c), C.byref(d), C.byref(e), C.byref(lut))
    return (r.w, r.h) if 0 < r.w and 0 < r.h and r.w * r.h <= (1 << 22) else (1, 1)


def test_one_mixed_batch_next_to_plain_calls(enc):
    """Formats, pitches, file channels, stored and compressed files in ONE call, with plain decode_device calls on the same encoder
    before and after: neither path disturbs the other's results."""
    import torch
    rng = np.random.default_rng(31)
    items = []
    for k in range(40):
        img, w, h, c = fuzz_image(rng)
        items.append((img.reshape(h, w, c), k % 3))
    pngs = _encode_gpu(enc, items)
    dims = [(im.shape[1], im.shape[0]) for im, _ in items]
    plain_dev = _device_files(pngs, shift=1)
    before = [(st, px.clone() if px is not None else None) for st, px, _ in enc.decode_device(plain_dev, 4, dims)]
    buf_parts, views, orders, ups, exp = [], [], [], [], []
    for i, ((w, h), png) in enumerate(zip(dims, pngs)):
        name, kind = NAMES[i % len(NAMES)], KINDS[(i // len(NAMES)) % 4]
        r = _Region(0, w, h, _nbytes(name), kind)
        b = torch.full((r.size,), SENTINEL, dtype=torch.uint8, device="cuda")
        buf_parts.append((b, r))
        views.append(_views(b, [r])[0])
        orders.append(name.lower())
        ups.append(kind == "bottom_up")
        cst, cpx, jw, jh, _ = judge(png, _nbytes(name))
        assert cst == 0
        exp.append(_reorder(np.asarray(cpx)[: w * h * _nbytes(name)].reshape(h, w, -1), name))
    got = enc.decode_device_ex(_device_files(pngs, shift=3), views, orders, ups)
    after = enc.decode_device(plain_dev, 4, dims)
    for i, ((st, v, _), (b, r)) in enumerate(zip(got, buf_parts)):
        assert st == 0, i
        host = b.cpu().numpy()
        for y in range(r.h):
            assert np.array_equal(host[r.row_offset(y): r.row_offset(y) + r.w * r.nb], exp[i][y].reshape(-1)), (i, y)
        assert _outside_untouched(host, [r]), i
    for i, ((st0, px0), (st1, px1, _)) in enumerate(zip(before, after)):
        assert st0 == st1 == 0 and torch.equal(px0, px1), i


def test_full_size_frames(enc):
    """8 x 8K RGBA into padded BGRA and bottom-up RGBA; 256 x 1080p RGB into BGR and RGBX -- against the packed path's output
    permuted with torch on the GPU."""
    import torch
    import fpng_amd
    w, h = 7680, 4320
    png8 = _encode_gpu(enc, [(fpng_amd.synth_image(("grad", "blocks")[k % 2], w, h, 4, seed=k), k % 2) for k in range(2)])
    pngs = [png8[k % 2] for k in range(8)]
    dev = _device_files(pngs)
    packed = [px for _, px, _ in enc.decode_device(dev, 4, [(w, h)] * 8)]
    pitch = w * 4 + 256
    big = torch.full((8, h, pitch), SENTINEL, dtype=torch.uint8, device="cuda")
    views = [big[k, :, : w * 4].view(h, w, 4) for k in range(8)]
    got = enc.decode_device_ex(dev, views, "bgra")
    assert all(st == 0 and v is views[k] for k, (st, v, _) in enumerate(got))
    for k in range(8):
        assert torch.equal(views[k], packed[k][..., [2, 1, 0, 3]]), k
    assert bool((big[:, :, w * 4:] == SENTINEL).all())
    up = [torch.empty((h, w, 4), dtype=torch.uint8, device="cuda") for _ in range(8)]
    got = enc.decode_device_ex(dev, up, "rgba", bottom_up=True)
    for k in range(8):
        assert got[k][0] == 0 and torch.equal(up[k], packed[k].flip(0)), k
    del big, views, up, packed
    w, h = 1920, 1080
    png1 = _encode_gpu(enc, [(fpng_amd.synth_image(("grad", "blocks", "noise")[k % 3], w, h, 3, seed=k), k % 2) for k in range(4)])
    pngs = [png1[k % 4] for k in range(256)]
    dev = _device_files(pngs)
    packed = [px for _, px, _ in enc.decode_device(dev, 3, [(w, h)] * 256)]
    bgr = [torch.empty((h, w, 3), dtype=torch.uint8, device="cuda") for _ in range(256)]
    got = enc.decode_device_ex(dev, bgr, "bgr")
    for k in range(256):
        assert got[k][0] == 0 and torch.equal(bgr[k], packed[k].flip(2)), k
    del bgr
    rgbx = [torch.empty((h, w, 4), dtype=torch.uint8, device="cuda") for _ in range(256)]
    got = enc.decode_device_ex(dev, rgbx, "rgbx")
    for k in range(256):
        assert got[k][0] == 0 and torch.equal(rgbx[k][..., :3], packed[k]) and bool((rgbx[k][..., 3] == 0xFF).all()), k


def _raw_call(enc, pngs, recs, device):
    """fpng_amd_decode_batch(_device)_ex on hand-made records: (rc, statuses)"""
    import torch
    from fpng_amd import _lib
    n = len(recs)
    arr = (_lib.PngExIn * n)()
    res = (_lib.DecodeResult * n)()
    keep = _device_files(pngs, shift=1) if device else [np.frombuffer(bytes(p), dtype=np.uint8) for p in pngs]
    for i, (fmt, ptr, pitch, cap) in enumerate(recs):
        arr[i].data = keep[i].data_ptr() if device else keep[i].ctypes.data
        arr[i].size = len(pngs[i])
        arr[i].format, arr[i].d_pixels, arr[i].row_pitch, arr[i].pixels_cap = fmt, ptr, pitch, cap
    fn = enc.lib.fpng_amd_decode_batch_device_ex if device else enc.lib.fpng_amd_decode_batch_ex
    enc._sync_stream()
    rc = fn(enc.h, arr, n, res)
    torch.cuda.synchronize()
    return rc, [r.status for r in res]


@pytest.mark.parametrize("device", [False, True])
def test_validation(enc, device):
    """Every rule gets its error code, the call writes nothing (the sentinel-filled buffers stay as they were -- also the valid
    file's in front of the bad one), and the next valid call succeeds."""
    import torch
    INVALID, SMALL = -1, -4
    w, h = 37, 21
    good = _encode_gpu(enc, [(np.random.default_rng(3).integers(0, 256, (h, w, 4), dtype=np.uint8), 0)])[0]
    broken = b"\x89PNG\r\n\x1a\n" + b"\0" * 40  # rejected by the container walk: needs no room
    buf = torch.full((1 << 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    base = buf.data_ptr()
    F = {n: i for i, n in enumerate(NAMES)}
    ok = (F["BGRA"], base, 0, w * h * 4)
    cases = [
        ((10, base + 8192, 0, 1 << 14), INVALID),                          # unknown format
        ((F["RGBA"], base + 8192 + 2, 0, 1 << 14), INVALID),               # 4-byte format, d_pixels not a multiple of 4
        ((F["XBGR"], base + 8192, w * 4 + 2, 1 << 14), INVALID),           # 4-byte format, pitch not a multiple of 4
        ((F["BGR"], base + 8192, w * 3 - 1, 1 << 14), INVALID),            # |pitch| < w * bytes
        ((F["RGBA"], base + 8192, -(w * 4 - 4), 1 << 14), INVALID),        # ... bottom-up too
        ((F["RGB"], base + 8192, 1 << 31, 1 << 14), INVALID),              # |pitch| >= 2^31
        ((F["RGBA"], base + 8192, 0, w * h * 4 - 1), SMALL),               # cap one byte short
        ((F["BGR"], base + 8193, w * 3 + 5, (h - 1) * (w * 3 + 5) + w * 3 - 1), SMALL),
        ((F["RGBA"], 0, 0, 1 << 14), SMALL),                               # no buffer
    ]
    for rec, code in cases:
        rc, _ = _raw_call(enc, [good, good], [ok, rec], device)
        assert rc == code, (rec, rc)
        assert bool((buf == SENTINEL).all()), rec
    # rules that hold: odd start and pitch for 3-byte formats, an exact cap, a bottom-up pitch, a rejected file without room
    rc, sts = _raw_call(enc, [good, good, good, broken], [ok, (F["BGR"], base + 8193, w * 3 + 5, (h - 1) * (w * 3 + 5) + w * 3),
                                                          (F["XRGB"], base + 16384 + (h - 1) * w * 4, -w * 4, w * h * 4), (F["RGBA"], 0, 0, 0)], device)
    assert rc == 0 and sts[:3] == [0, 0, 0] and sts[3] != 0, (rc, sts)
    cst, cpx, *_ = judge(good, 4)
    px = np.asarray(cpx)[: w * h * 4].reshape(h, w, 4)
    host = buf.cpu().numpy()
    assert np.array_equal(host[: w * h * 4].reshape(h, w, 4), _reorder(px, "BGRA"))
    got3 = np.stack([host[8193 + y * (w * 3 + 5): 8193 + y * (w * 3 + 5) + w * 3] for y in range(h)]).reshape(h, w, 3)
    assert np.array_equal(got3, _reorder(px[..., :3], "BGR"))
    assert np.array_equal(host[16384: 16384 + w * h * 4].reshape(h, w, 4)[::-1], _reorder(px, "XRGB"))
    assert host[w * h * 4] == SENTINEL and host[8192] == SENTINEL


def test_a_descriptor_decodes_again_after_its_outputs_are_overwritten(enc):
    """make_decode_batch_ex(): built once, called again after the outputs were overwritten -- the same pixels."""
    import torch
    rng = np.random.default_rng(41)
    items = []
    for k in range(24):
        img, w, h, c = fuzz_image(rng)
        items.append((img.reshape(h, w, c), k % 3))
    pngs = _encode_gpu(enc, items)
    outs, orders = [], []
    for i, (im, _) in enumerate(items):
        h, w, _c = im.shape
        name = NAMES[i % len(NAMES)]
        orders.append(name.lower())
        outs.append(torch.empty((h, w, _nbytes(name)), dtype=torch.uint8, device="cuda"))
    db = enc.make_decode_batch_ex(_device_files(pngs, shift=2), outs, orders, [i % 2 == 1 for i in range(24)])
    first = [(st, v.clone()) for st, v, _ in enc.decode_device_ex(db)]
    for t in outs:
        t.fill_(0x3C)
    assert enc.decode_device_ex(db, results=False) is db
    assert list(db.statuses()) == [0] * 24
    for i, ((st, v0), (st2, v1, _)) in enumerate(zip(first, db.results())):
        assert st == st2 == 0 and v1 is outs[i] and torch.equal(v0, v1), i
        name = NAMES[i % len(NAMES)]
        cst, cpx, w, h, _ = judge(pngs[i], _nbytes(name))
        exp = _reorder(np.asarray(cpx)[: w * h * _nbytes(name)].reshape(h, w, -1), name)
        assert np.array_equal(v1.cpu().numpy(), exp[::-1] if i % 2 else exp), i
    hb = enc.make_decode_batch_ex(pngs, outs, orders)
    with pytest.raises(ValueError):
        enc.decode_device_ex(hb)  # (host files: decode_batch_ex)
    assert [st for st, _, _ in enc.decode_batch_ex(hb)] == [0] * 24


def test_torch_views_are_filled_in_place(enc):
    """A crop big[y0:y0+h, x0:x0+w, :] of a larger channels-last tensor, a bottom_up=True target and a BGRA view: filled in place,
    the results are the caller's own tensors, and the crop's surroundings are untouched."""
    import torch
    rng = np.random.default_rng(51)
    h, w = 45, 70
    img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    img[:, :, :2] = (np.arange(w, dtype=np.uint8)[None, :, None] // 3)  # something compressible
    png = _encode_gpu(enc, [(img, 0)])[0]
    big = torch.full((200, 300, 4), SENTINEL, dtype=torch.uint8, device="cuda")
    y0, x0 = 33, 101
    crop = big[y0:y0 + h, x0:x0 + w, :]
    ptr = crop.data_ptr()
    (st, v, cf), = enc.decode_batch_ex([png], [crop], "rgba")
    assert st == 0 and cf == 4 and v is crop and crop.data_ptr() == ptr
    assert np.array_equal(crop.cpu().numpy(), img)
    outside = big.clone()
    outside[y0:y0 + h, x0:x0 + w, :] = SENTINEL
    assert bool((outside == SENTINEL).all())
    gl = torch.full((h, w, 4), SENTINEL, dtype=torch.uint8, device="cuda")
    (st, v, _), = enc.decode_device_ex(_device_files([png], shift=1), [gl], "rgba", bottom_up=True)
    assert st == 0 and v is gl and np.array_equal(gl.cpu().numpy(), img[::-1])
    bgra = torch.full((h, w, 4), SENTINEL, dtype=torch.uint8, device="cuda")
    (st, v, _), = enc.decode_device_ex(_device_files([png]), [bgra], "bgra")
    assert st == 0 and v is bgra and np.array_equal(bgra.cpu().numpy(), img[..., [2, 1, 0, 3]])
