"""GPU decoder into planar (channels-first, CHW) device images (-m gpu; fpng_amd_decode_batch_planar /
fpng_amd_decode_batch_device_planar, dec_unfilter_planar_kernel and dec_stored_planar_kernel): three and four planes, every pitch
kind, against the REFERENCE's decoder at desired 3 or 4 split into planes in numpy, statuses against the packed call, and not one
byte written outside the c * h spans of w bytes."""
import os
import struct

import numpy as np
import pytest

from cpu_ref import fuzz_image
from test_gpu_decode import UNDECIDED, _device_files, judge
from test_gpu_decode_layouts import SENTINEL, _damaged_files, _encode_gpu, _header_dims, _matrix_files

pytestmark = pytest.mark.gpu

KINDS = ["packed", "odd", "pad256", "bottom_up", "reversed"]


@pytest.fixture(scope="module")
def enc(built_lib):
    import torch
    import fpng_amd
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    e = fpng_amd.Encoder(device=0)
    yield e
    e.close()


class _Region:
    """a file's destination inside one sentinel-filled buffer: a margin, c planes `pp` bytes apart of h rows `rp` bytes apart, a margin"""

    def __init__(self, off, w, h, c, kind):
        self.w, self.h, self.c, self.kind = w, h, c, kind
        self.rp = w + {"odd": 7 - (w & 1), "pad256": 256}.get(kind, 0)  # (odd: an odd pitch from an odd byte)
        self.pp = h * self.rp + {"odd": 5 + ((h * self.rp) & 1), "reversed": 9, "pad256": 64}.get(kind, 0)
        self.front = 64 + (1 if kind == "odd" else 0)
        self.off = off  # the region's first byte (4-byte aligned)
        self.lo = off + self.front  # the lowest-addressed row's first byte
        self.span = (c - 1) * self.pp + (h - 1) * self.rp + w
        self.size = (self.front + self.span + 64 + 3) & ~3

    def row_offset(self, ch, y):  # where row y of the file's channel ch lies
        slot = (self.c - 1 - ch) if self.kind == "reversed" else ch
        return self.lo + slot * self.pp + ((self.h - 1 - y) if self.kind == "bottom_up" else y) * self.rp

    def order(self):
        return ("bgr" if self.c == 3 else "abgr") if self.kind == "reversed" else ("rgb" if self.c == 3 else "rgba")

    def view(self, buf):  # the (c, h, w) tensor view a caller holds (planes in memory order)
        return buf.as_strided((self.c, self.h, self.w), (self.pp, self.rp, 1), self.lo)

    def put(self, exp, px):  # px (h, w, c) in R,G,B[,A] order into the expected buffer
        for ch in range(self.c):
            for y in range(self.h):
                exp[self.row_offset(ch, y): self.row_offset(ch, y) + self.w] = px[y, :, ch]

    def spans(self):
        return [(self.row_offset(ch, y), self.row_offset(ch, y) + self.w) for ch in range(self.c) for y in range(self.h)]


def _regions(dims, c, kinds):
    regs, off = [], 0
    for (w, h), kind in zip(dims, kinds):
        r = _Region(off, max(w, 1), max(h, 1), c, kind)
        regs.append(r)
        off += r.size
    return regs, off


def _decode_planar(enc, pngs, regs, total, device):
    """one call into ONE sentinel-filled buffer: (results, the buffer's bytes afterwards, the views)"""
    import torch
    buf = torch.full((total,), SENTINEL, dtype=torch.uint8, device="cuda")
    views = [r.view(buf) for r in regs]
    orders, ups = [r.order() for r in regs], [r.kind == "bottom_up" for r in regs]
    if device:
        got = enc.decode_device_planar(_device_files(pngs, shift=1), views, orders, ups)
    else:
        got = enc.decode_batch_planar(pngs, views, orders, ups)
    torch.cuda.synchronize()
    return got, buf.cpu().numpy(), views


def _outside_untouched(host, regs):
    mask = np.ones(host.size, dtype=bool)
    for r in regs:
        for a, b in r.spans():
            mask[a:b] = False
    return bool(np.all(host[mask] == SENTINEL))


@pytest.fixture(scope="module")
def matrix(enc):
    pngs = _matrix_files(enc)
    judged = {d: [judge(p, d) for p in pngs] for d in (3, 4)}
    packed = {d: enc.decode_batch(pngs, d) for d in (3, 4)}
    return pngs, judged, packed


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("c", [3, 4])
def test_every_pitch_and_width(enc, matrix, c, device):
    """3- and 4-channel files x 1-pass, 2-pass and stored x widths around the epilogue's edges (1 ... 257, 7680) x heights around the
    48-row segment x pitch kinds dealt round-robin, into three and four planes, one call per plane count and entry point into ONE
    buffer that is compared WHOLE: the reference's pixels, the packed call's statuses (all 0), not a byte outside the spans."""
    pngs, judged, packed = matrix
    dims = [struct.unpack(">II", bytes(p[16:24])) for p in pngs]
    kinds = [KINDS[i % len(KINDS)] for i in range(len(pngs))]
    regs, total = _regions(dims, c, kinds)
    got, host, views = _decode_planar(enc, pngs, regs, total, device)
    exp = np.full(total, SENTINEL, dtype=np.uint8)
    for i, (png, r, (st, view, cf)) in enumerate(zip(pngs, regs, got)):
        cst, cpx, w, h, fc = judged[c][i]
        pst, _, pcf = packed[c][i]
        assert st == cst == pst == 0 and cf == fc == pcf, (i, st, cst, pst)
        assert view is views[i]
        r.put(exp, np.asarray(cpx)[: w * h * c].reshape(h, w, c))
    bad = np.nonzero(host != exp)[0]
    assert bad.size == 0, (c, device, bad.size, int(bad[0]), [(i, r.w, r.h, r.kind, int(bad[0]) - r.lo) for i, r in enumerate(regs) if r.off <= bad[0] < r.off + r.size])


@pytest.mark.parametrize("device", [False, True])
def test_damaged_and_undecided_files_write_nothing_outside_the_spans(enc, device):
    """container_mutator / token_mutator files, and every compressed file UNDECIDED (FPNG_AMD_DECODE_MAX_ROUNDS=0): each status and
    channels_in_file is the packed call's at the same desired channels, and every byte outside the spans keeps its sentinel."""
    pngs = _damaged_files()
    dims = [_header_dims(p) for p in pngs]
    kinds = [KINDS[i % len(KINDS)] for i in range(len(pngs))]
    for c in (3, 4):
        for forced in (False, True):
            if forced:
                os.environ["FPNG_AMD_DECODE_MAX_ROUNDS"] = "0"
            try:
                packed = enc.decode_batch(pngs, c)
                regs, total = _regions(dims, c, kinds)
                got, host, _ = _decode_planar(enc, pngs, regs, total, device)
            finally:
                if forced:
                    del os.environ["FPNG_AMD_DECODE_MAX_ROUNDS"]
            sts = [st for st, _, _ in got]
            assert sts == [st for st, _, _ in packed], (c, forced)
            assert [cf for _, _, cf in got] == [cf for _, _, cf in packed], (c, forced)
            if forced:
                assert UNDECIDED in sts
            assert any(st not in (0, UNDECIDED) for st in sts)
            assert _outside_untouched(host, regs), (c, forced, device)


def test_one_mixed_batch_next_to_plain_calls(enc):
    """Plane counts, pitches, file channels, stored and compressed files in ONE call, with plain decode_device calls on the same
    encoder before and after: neither path disturbs the other's results."""
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
    parts, views, exp = [], [], []
    for i, ((w, h), png) in enumerate(zip(dims, pngs)):
        c, kind = 3 + (i & 1), KINDS[(i // 2) % len(KINDS)]
        r = _Region(0, w, h, c, kind)
        b = torch.full((r.size,), SENTINEL, dtype=torch.uint8, device="cuda")
        parts.append((b, r))
        views.append(r.view(b))
        cst, cpx, jw, jh, _ = judge(png, c)
        assert cst == 0
        e = np.full(r.size, SENTINEL, dtype=np.uint8)
        r.put(e, np.asarray(cpx)[: w * h * c].reshape(h, w, c))
        exp.append(e)
    got = enc.decode_device_planar(_device_files(pngs, shift=3), views, [r.order() for _, r in parts], [r.kind == "bottom_up" for _, r in parts])
    after = enc.decode_device(plain_dev, 4, dims)
    for i, ((st, v, _), (b, r)) in enumerate(zip(got, parts)):
        assert st == 0 and v is views[i], i
        assert np.array_equal(b.cpu().numpy(), exp[i]), (i, r.w, r.h, r.c, r.kind)
    for i, ((st0, px0), (st1, px1, _)) in enumerate(zip(before, after)):
        assert st0 == st1 == 0 and torch.equal(px0, px1), i


def test_full_size_frames(enc):
    """8 x 8K RGBA into CHW (four planes, and three) and 256 x 1080p RGB into one NCHW tensor (three planes, and four) -- against the
    packed path's output permuted with torch on the GPU (the existing tests pin that path to the reference)."""
    import torch
    import fpng_amd
    w, h = 7680, 4320
    png8 = _encode_gpu(enc, [(fpng_amd.synth_image(("grad", "blocks")[k % 2], w, h, 4, seed=k), k % 2) for k in range(2)])
    pngs = [png8[k % 2] for k in range(8)]
    dev = _device_files(pngs)
    packed = [px for _, px, _ in enc.decode_device(dev, 4, [(w, h)] * 8)]
    nchw = torch.full((8, 4, h, w), SENTINEL, dtype=torch.uint8, device="cuda")
    got = enc.decode_device_planar(dev, list(nchw))
    for k in range(8):
        assert got[k][0] == 0 and got[k][2] == 4 and torch.equal(nchw[k], packed[k].permute(2, 0, 1)), k
    nchw.fill_(SENTINEL)
    got = enc.decode_device_planar(dev, [nchw[k, :3] for k in range(8)])
    for k in range(8):
        assert got[k][0] == 0 and torch.equal(nchw[k, :3], packed[k][..., :3].permute(2, 0, 1)), k
    assert bool((nchw[:, 3] == SENTINEL).all()), "three planes of a four-plane tensor: the fourth is not the decoder's"
    del nchw, packed
    w, h = 1920, 1080
    png1 = _encode_gpu(enc, [(fpng_amd.synth_image(("grad", "blocks", "noise")[k % 3], w, h, 3, seed=k), k % 2) for k in range(4)])
    pngs = [png1[k % 4] for k in range(256)]
    dev = _device_files(pngs)
    packed = [px for _, px, _ in enc.decode_device(dev, 3, [(w, h)] * 256)]
    nchw = torch.full((256, 3, h, w), SENTINEL, dtype=torch.uint8, device="cuda")
    got = enc.decode_device_planar(dev, list(nchw))
    for k in range(256):
        assert got[k][0] == 0 and got[k][2] == 3 and torch.equal(nchw[k], packed[k].permute(2, 0, 1)), k
    del nchw
    n4 = torch.full((256, 4, h, w), SENTINEL, dtype=torch.uint8, device="cuda")
    got = enc.decode_device_planar(dev, list(n4))
    for k in range(256):
        assert got[k][0] == 0 and torch.equal(n4[k, :3], packed[k].permute(2, 0, 1)) and bool((n4[k, 3] == 0xFF).all()), k


def _raw_call(enc, pngs, recs, device):
    """fpng_amd_decode_batch(_device)_planar on hand-made records (num_chans, d_pixels, row_pitch, plane_pitch, cap): (rc, statuses)"""
    import torch
    from fpng_amd import _lib
    n = len(recs)
    arr = (_lib.PngPlanarIn * n)()
    res = (_lib.DecodeResult * n)()
    keep = _device_files(pngs, shift=1) if device else [np.frombuffer(bytes(p), dtype=np.uint8) for p in pngs]
    for i, (c, ptr, rp, pp, cap) in enumerate(recs):
        arr[i].data = keep[i].data_ptr() if device else keep[i].ctypes.data
        arr[i].size = len(pngs[i])
        arr[i].num_chans, arr[i].d_pixels, arr[i].row_pitch, arr[i].plane_pitch, arr[i].pixels_cap = c, ptr, rp, pp, cap
    fn = enc.lib.fpng_amd_decode_batch_device_planar if device else enc.lib.fpng_amd_decode_batch_planar
    enc._sync_stream()
    rc = fn(enc.h, arr, n, res)
    torch.cuda.synchronize()
    return rc, [r.status for r in res]


@pytest.mark.parametrize("device", [False, True])
def test_validation(enc, device):
    """Every rule gets its error code, the call writes nothing (the sentinel-filled buffer stays as it was -- also the valid file's
    part in front of the bad one), and the next valid call succeeds."""
    import torch
    INVALID, SMALL = -1, -4
    w, h = 37, 21
    good = _encode_gpu(enc, [(np.random.default_rng(3).integers(0, 256, (h, w, 4), dtype=np.uint8), 0)])[0]
    broken = b"\x89PNG\r\n\x1a\n" + b"\0" * 40  # rejected by the container walk: needs no room
    buf = torch.full((1 << 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    base = buf.data_ptr()
    full = 3 * w * h + (h - 1) * w + w  # span of four packed planes
    ok = (4, base, 0, 0, full)
    rp, pp = w + 3, h * (w + 3) + 2
    span3 = 2 * pp + (h - 1) * rp + w
    cases = [
        ((2, base + 8192, 0, 0, 1 << 14), INVALID),                        # num_chans
        ((5, base + 8192, 0, 0, 1 << 14), INVALID),
        ((4, base + 8192, w - 1, 0, 1 << 14), INVALID),                    # |row_pitch| < w
        ((4, base + 8192 + (h - 1) * w, -(w - 1), h * w, 1 << 14), INVALID),  # ... bottom-up too
        ((3, base + 8192, 1 << 31, 0, 1 << 14), INVALID),                  # |row_pitch| >= 2^31
        ((3, base + 8192, -(1 << 31), 0, 1 << 14), INVALID),
        ((4, base + 8192, w, h * w - 1, 1 << 14), INVALID),                # planes overlap
        ((3, base + 8192 + 2 * h * w, w, -(h * w - 1), 1 << 14), INVALID),  # ... in reverse order too
        ((3, base + 8192, w + 8, h * w, 1 << 14), INVALID),                # ... because of the rows' padding
        ((4, base + 8192, 0, 0, full - 1), SMALL),                         # cap one byte short
        ((3, base + 8193, rp, pp, span3 - 1), SMALL),
        ((4, 0, 0, 0, 1 << 14), SMALL),                                    # no buffer
    ]
    for rec, code in cases:
        rc, _ = _raw_call(enc, [good, good], [ok, rec], device)
        assert rc == code, (rec, rc)
        assert bool((buf == SENTINEL).all()), rec
    # rules that hold: any start byte and pitch, an exact cap, negative pitches of both kinds, a rejected file without room
    o3, o4 = 8193, 16384
    rc, sts = _raw_call(enc, [good, good, good, broken],
                        [ok, (3, base + o3, rp, pp, span3), (4, base + o4 + 3 * h * w + (h - 1) * w, -w, -h * w, full), (4, 0, 0, 0, 0)], device)
    assert rc == 0 and sts[:3] == [0, 0, 0] and sts[3] != 0, (rc, sts)
    cst, cpx, *_ = judge(good, 4)
    px = np.asarray(cpx)[: w * h * 4].reshape(h, w, 4)
    host = buf.cpu().numpy()
    exp = np.full(host.size, SENTINEL, dtype=np.uint8)
    exp[: 4 * h * w] = px.transpose(2, 0, 1).reshape(-1)
    for ch in range(3):
        for y in range(h):
            exp[o3 + ch * pp + y * rp: o3 + ch * pp + y * rp + w] = px[y, :, ch]
    exp[o4: o4 + 4 * h * w] = px.transpose(2, 0, 1)[::-1, ::-1].reshape(-1)  # planes A,B,G,R, rows bottom-up
    assert np.array_equal(host, exp)


def test_a_descriptor_decodes_again_after_its_outputs_are_overwritten(enc):
    """make_decode_batch_planar(): built once, called again after the outputs were overwritten -- the same pixels."""
    import torch
    rng = np.random.default_rng(41)
    items = []
    for k in range(24):
        img, w, h, c = fuzz_image(rng)
        items.append((img.reshape(h, w, c), k % 3))
    pngs = _encode_gpu(enc, items)
    outs = [torch.empty((3 + (i & 1), im.shape[0], im.shape[1]), dtype=torch.uint8, device="cuda") for i, (im, _) in enumerate(items)]
    ups = [i % 3 == 1 for i in range(24)]
    db = enc.make_decode_batch_planar(_device_files(pngs, shift=2), outs, "rgb", ups)
    first = [(st, v.clone()) for st, v, _ in enc.decode_device_planar(db)]
    for t in outs:
        t.fill_(0x3C)
    assert enc.decode_device_planar(db, results=False) is db
    assert list(db.statuses()) == [0] * 24
    for i, ((st, v0), (st2, v1, _)) in enumerate(zip(first, db.results())):
        assert st == st2 == 0 and v1 is outs[i] and torch.equal(v0, v1), i
        c = 3 + (i & 1)
        cst, cpx, w, h, _ = judge(pngs[i], c)
        exp = np.asarray(cpx)[: w * h * c].reshape(h, w, c).transpose(2, 0, 1)
        assert np.array_equal(v1.cpu().numpy(), exp[:, ::-1] if ups[i] else exp), i
    hb = enc.make_decode_batch_planar(pngs, outs, "rgb", ups)
    with pytest.raises(ValueError):
        enc.decode_device_planar(hb)  # (host files: decode_batch_planar)
    assert [st for st, _, _ in enc.decode_batch_planar(hb)] == [0] * 24


def test_torch_views_are_filled_in_place(enc):
    """A crop big[:, y0:y0+h, x0:x0+w] of a larger CHW tensor and nchw[i]: filled in place, the results are the caller's own tensors,
    and the surroundings are untouched."""
    import torch
    rng = np.random.default_rng(51)
    h, w = 45, 71
    img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    img[:, :, :2] = (np.arange(w, dtype=np.uint8)[None, :, None] // 3)  # something compressible
    png = _encode_gpu(enc, [(img, 0)])[0]
    chw = np.ascontiguousarray(img.transpose(2, 0, 1))
    big = torch.full((4, 200, 301), SENTINEL, dtype=torch.uint8, device="cuda")
    y0, x0 = 33, 101
    crop = big[:, y0:y0 + h, x0:x0 + w]
    (st, v, cf), = enc.decode_batch_planar([png], [crop])
    assert st == 0 and cf == 4 and v is crop
    assert np.array_equal(crop.cpu().numpy(), chw)
    outside = big.clone()
    outside[:, y0:y0 + h, x0:x0 + w] = SENTINEL
    assert bool((outside == SENTINEL).all())
    nchw = torch.full((3, 3, h, w), SENTINEL, dtype=torch.uint8, device="cuda")
    (st, v, _), = enc.decode_device_planar(_device_files([png], shift=1), [nchw[1]])
    assert st == 0 and v.data_ptr() == nchw[1].data_ptr() and np.array_equal(nchw[1].cpu().numpy(), chw[:3])
    assert bool((nchw[0] == SENTINEL).all()) and bool((nchw[2] == SENTINEL).all())
    bgr = torch.full((3, h, w), SENTINEL, dtype=torch.uint8, device="cuda")
    (st, v, _), = enc.decode_device_planar(_device_files([png]), [bgr], "bgr", bottom_up=True)
    assert st == 0 and v is bgr and np.array_equal(bgr.cpu().numpy(), chw[:3][::-1, ::-1])
    with pytest.raises(ValueError):
        enc.decode_batch_planar([png], [bgr.cpu()])


def test_round_trip_chw(enc):
    """CHW tensor -> submit_planar -> decode_device_planar -> the same tensor, 1-pass, 2-pass and stored, three and four planes."""
    import torch
    import fpng_amd
    g = torch.Generator(device="cpu").manual_seed(7)
    for c, (h, w) in ((3, (211, 333)), (4, (97, 1025)), (3, (1, 1)), (4, (50, 7))):
        src = torch.randint(0, 256, (c, h, w), dtype=torch.uint8, generator=g)
        src[:, :, : w // 2] = src[:, :1, : w // 2]  # (half of every row repeats the first row: something for the filter)
        src = src.cuda()
        for flags in (0, 1, 2):
            out = torch.empty(fpng_amd.max_encoded_size(w, h, c) + 64, dtype=torch.uint8, device="cuda")
            enc.submit_planar([src], [out], flags)
            (size, mode, status), = enc.wait(enc.last_ticket, 1)
            assert status == 0
            back = torch.full((c, h, w), SENTINEL, dtype=torch.uint8, device="cuda")
            (st, v, cf), = enc.decode_device_planar([out[:size].clone()], [back])
            assert st == 0 and cf == c and torch.equal(back, src), (c, h, w, flags)
