"""GPU tests (-m gpu) of walk_row's instantiations for the source layouts OTHER than plain packed pixels -- fpng_amd_encode_submit_ex
(C3/L3, C3/L4, C4/L4), _planar (C3, C4) and _planar_float (f32 / f16 / bf16 x C3, C4), Pass::Hist and Pass::Encode of each -- with
the content that is delicate for the walk: tests/walk_cases.layout_battery, about 300 images of at most 2065 x 5 pixels per channel
count that reach every tier, row end, hand-over and seam of the walk (tests/test_walk_cases_cpu.py proves that, without a GPU).

The judge is test_gpu_layouts' (the reference's file if the reference is built, else the oracle's), computed once per image and
flag; every comparison is the whole file.  Every source buffer is RANDOM wherever it is not a pixel -- X bytes, row padding, the gap
behind a plane, the unused fourth plane -- and must be unchanged afterwards.  The float sources hold integers (byte, or byte - 128
with a bias of 128): exact in all three dtypes (test_walk_cases_cpu.test_float_sources_are_exact), so the expected bytes are the
image's own."""
import time

import numpy as np
import pytest

import walk_cases as W
from cpu_ref import have_ref, ref
from test_gpu_layouts import _expect, _fmt, _layout, _same, _submit_raw as _submit_ex, _to_source
from test_gpu_planar import _submit_raw as _submit_planar
from test_gpu_float_encode import _submit_raw as _submit_float

pytestmark = pytest.mark.gpu

ELEM = {0: 4, 1: 2, 2: 2}
DTYPE_NAMES = {0: "f32", 1: "f16", 2: "bf16"}
# (kind, ...): ("ex", format) | ("planar", c) | ("float", code, c, set)
SOURCES = ([("ex", n) for n in W.EX_FORMATS] + [("planar", 3), ("planar", 4)] +
           [("float", code, c, s) for code in (0, 1, 2) for c in (3, 4) for s in W.FLOAT_SETS])


def _sid(src):
    if src[0] == "float":
        return f"{DTYPE_NAMES[src[1]]}_c{src[2]}_{src[3]}"
    return "_".join(str(v) for v in src)


def _chans(src):
    return _fmt(src[1])[2] if src[0] == "ex" else src[1] if src[0] == "planar" else src[2]


@pytest.fixture(scope="module")
def enc(built_lib):
    import torch
    import fpng_amd
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    e = fpng_amd.Encoder(device=0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def expected():
    """the judge's file for (image, flags), made once per module"""
    made = {}

    def get(img, flags):
        key = (img.shape, img.tobytes(), flags)
        if key not in made:
            made[key] = _expect(img, flags)
        return made[key]
    return get


class Staged:
    """The source buffers of a list of images in ONE host array (each on a 16-byte boundary) and its copy on the device.
    rows[i]: byte offsets (planes, h) of every plane row of image i inside the array (packed sources: one "plane")."""

    def __init__(self, src, imgs, seed=1):
        fill = np.random.default_rng([seed, len(imgs)] + [ord(ch) for ch in _sid(src)])
        parts, self.rows, self.geo, pos = [], [], [], 0
        for i, img in enumerate(imgs):
            h, w, c = img.shape
            if src[0] == "ex":
                v, sb, _ = _fmt(src[1])
                buf, top, pitch = _layout(_to_source(img, src[1], fill), W.ex_pitch_kind(i, sb), fill)
                geo, rows = (top, pitch, w, h, v), (top + pitch * np.arange(h))[None, :]
            else:
                code = src[1] if src[0] == "float" else None
                e = ELEM[code] if code is not None else 1
                vals = img if code is None else W.float_bits(img, code, W.FLOAT_SETS[src[3]][0])
                buf, top, rp, pp = W.planes(vals, W.planar_kind(i, c), fill)
                buf = buf.view(np.uint8)
                geo, rows = (top * e, rp * e, pp * e, w, h, c), W.plane_row_offsets(top, rp, pp, h, c) * e
            parts.append((pos, buf))
            self.geo.append((pos,) + geo)
            self.rows.append(rows + pos)
            pos += (len(buf) + 15) & ~15
        self.host = np.empty(pos, dtype=np.uint8)
        self.host[:] = fill.integers(0, 256, pos, dtype=np.uint8)
        for o, buf in parts:
            self.host[o:o + len(buf)] = buf
        self.src, self.imgs, self._dev = src, imgs, None

    @property
    def dev(self):
        if self._dev is None:
            import torch
            self._dev = torch.from_numpy(self.host).cuda()
            assert self._dev.data_ptr() % 16 == 0
        return self._dev

    def submit(self, enc, flags):
        """one submission of all images, not waited for -> (ticket, output tensor, [(offset, capacity)])"""
        import torch
        import fpng_amd
        src, caps, pos = self.src, [], 0
        for img in self.imgs:
            cap = fpng_amd.max_encoded_size(img.shape[1], img.shape[0], img.shape[2]) + 64
            caps.append((pos, cap))
            pos += (cap + 255) & ~255
        out = torch.empty(pos, dtype=torch.uint8, device="cuda")
        base, obase = self.dev.data_ptr(), out.data_ptr()
        if src[0] == "ex":
            descs = [(base + p + top, pitch, w, h, v, obase + o, cap) for (p, top, pitch, w, h, v), (o, cap) in zip(self.geo, caps)]
            rc, t = _submit_ex(enc, descs, flags)
        else:
            descs = [(base + p + top, rp, pp, w, h, c, 0, obase + o, cap) for (p, top, rp, pp, w, h, c), (o, cap) in zip(self.geo, caps)]
            if src[0] == "planar":
                rc, t = _submit_planar(enc, descs, flags)
            else:
                _, scale, bias = W.FLOAT_SETS[src[3]]
                rc, t = _submit_float(enc, descs, src[1], [scale] * 4, [bias] * 4, flags)
        assert rc == 0 and t, enc.lib.fpng_amd_last_error()
        return t, out, caps

    def collect(self, enc, t, out, caps):
        """-> [file bytes]; every status 0, the source unchanged"""
        res = enc.wait(t, len(self.imgs))
        host = out.cpu().numpy()
        files = []
        for (size, mode, status), (o, cap) in zip(res, caps):
            assert status == 0 and size <= cap
            files.append(host[o:o + size].tobytes())
        assert len(files) == len(self.imgs)
        assert np.array_equal(self.dev.cpu().numpy(), self.host), f"{_sid(self.src)}: the submission wrote into the source buffer"
        return files


@pytest.fixture(scope="module")
def staged():
    """source -> the battery staged in that layout, built once for both flags"""
    made = {}

    def get(src):
        if src not in made:
            made[src] = Staged(src, [img for _, img in W.layout_battery(_chans(src))])
        return made[src]
    return get


def _assert_phases(src, st):
    """what the battery's addresses must cover for this source, read from the descriptors: the phases count where the super-windows
    align with them, so among the rows of more than 256 pixels"""
    wide = [r for r, img in zip(st.rows, st.imgs) if img.shape[1] > 256]
    if src[0] == "ex" and _fmt(src[1])[1] == 3:
        rows = [r[0] for r in wide]
        assert {int(a) % 4 for r in rows for a in r} == {0, 1, 2, 3}, "3-byte rows: a byte phase is missing"
        assert {int(a) % 4 for r in rows for a in r[:-1]} == {0, 1, 2, 3}, "3-byte rows above: a byte phase is missing"
    elif src[0] == "planar":
        c = src[1]
        for ch in range(c):
            assert {int(a) % 4 for r in wide for a in r[ch]} == {0, 1, 2, 3}, f"plane {ch}: a byte phase of the row is missing"
            assert {int(a) % 4 for r in wide for a in r[ch][:-1]} == {0, 1, 2, 3}, f"plane {ch}: a byte phase of the row above is missing"
        n_phases = 0
        for i, r in enumerate(st.rows):
            if W.planar_kind(i, c) == "phases":
                n_phases += 1
                assert len({int(a) % 4 for a in r[:, 0]}) == c, "phases: two planes start at the same byte mod 4"
                assert all(int(a) % 4 != int(b) % 4 for ch in range(c) for a, b in zip(r[ch][1:], r[ch][:-1]))
        assert n_phases >= 40
    elif src[0] == "float" and ELEM[src[1]] == 2:
        for ch in range(src[2]):
            assert {int(a) % 4 for r in wide for a in r[ch]} == {0, 2}, f"plane {ch}: a dword phase of the row is missing"
            assert {int(a) % 4 for r in wide for a in r[ch][:-1]} == {0, 2}, f"plane {ch}: a dword phase of the row above is missing"
            assert {(int(a) % 4, int(b) % 4) for r in wide for a, b in zip(r[ch][1:], r[ch][:-1])} == {(0, 0), (0, 2), (2, 0), (2, 2)}


@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("src", SOURCES, ids=_sid)
def test_battery_every_source_both_passes(enc, staged, expected, src, flags):
    """The whole battery in ONE submission per source and flag: flags 0 runs Pass::Encode of the source's walk, flags 1
    (FPNG_ENCODE_SLOWER) Pass::Hist in front of it."""
    t0 = time.perf_counter()
    st = staged(src)
    _assert_phases(src, st)
    t1 = time.perf_counter()
    files = st.collect(enc, *st.submit(enc, flags))
    t2 = time.perf_counter()
    names = [n for n, _ in W.layout_battery(_chans(src))]
    for name, img, png in zip(names, st.imgs, files):
        _same(png, expected(img, flags), f"{_sid(src)} flags {flags}, battery image '{name}' {img.shape[1]}x{img.shape[0]}")
    print(f"\n{_sid(src)} flags {flags}: {len(files)} images; staging {t1 - t0:.2f} s, GPU {t2 - t1:.2f} s, judge and compare {time.perf_counter() - t2:.2f} s")


FLIP_SOURCES = {3: [("ex", "BGR"), ("ex", "XBGR"), ("planar", 3), ("float", 1, 3, "biased")],
                4: [("ex", "ABGR"), ("planar", 4), ("float", 0, 4, "biased")]}


@pytest.mark.skipif(not have_ref(), reason="the reference decides where the outcome flips")
@pytest.mark.parametrize("shape", [(256, 9, 4), (1024, 3, 3), (61, 17, 3)], ids=lambda s: "%dx%dx%d" % s)
def test_flip_point_through_every_source(enc, shape):
    """test_gpu_parity's stored-or-compressed sweep (first K pixels noise, the rest flat; K over the point where the reference's
    outcome flips, +-12) through one source per instantiation.  The decision hangs on the size of the row's final flush unit, which
    every layout computes in its own code: the row_end super-window (w = 256, 1024) reads n[3] of lane 63, the masked tail (w = 61)
    lane (w - 1) & 63.  Every file identical, both outcomes present."""
    w, h, c = shape
    rng = np.random.default_rng(2718 + w * 31 + h)
    noise = rng.integers(0, 256, (w * h, c), dtype=np.uint8)
    stored = lambda png: (png[60] >> 1) & 3 == 0

    def make(k):
        img = np.full((w * h, c), 77, dtype=np.uint8)
        img[:k] = noise[:k]
        return img.reshape(h, w, c)
    for flags in (0, 1):
        lo, hi = 0, w * h
        assert stored(ref().encode(make(hi), w, h, c, flags)) and not stored(ref().encode(make(0), w, h, c, flags))
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (lo, mid) if stored(ref().encode(make(mid), w, h, c, flags)) else (mid, hi)
        ks = list(range(max(0, hi - 12), min(w * h, hi + 12) + 1))
        imgs = [make(k) for k in ks]
        exps = [ref().encode(i, w, h, c, flags) for i in imgs]
        assert {stored(e) for e in exps} == {False, True}
        for src in FLIP_SOURCES[c]:
            st = Staged(src, imgs, seed=2)
            files = st.collect(enc, *st.submit(enc, flags))
            for k, png, exp in zip(ks, files, exps):
                _same(png, exp, f"{_sid(src)} {w}x{h}x{c} flags {flags}, K = {k} (flip at {hi})")


@pytest.mark.parametrize("c", [3, 4])
def test_mixed_sources_in_flight(enc, expected, c):
    """The battery's first 40 images as a plain, an _ex, a planar and a float submission back to back, none waited for until all
    are in flight: the scratch streams of one submission are the next one's neighbours."""
    import torch
    import fpng_amd
    imgs = [img for _, img in W.layout_battery(c)[:40]]
    sources = [("ex", "BGR" if c == 3 else "ABGR"), ("planar", c), ("float", 2 - (c & 1), c, "biased")]
    sts = [Staged(s, imgs, seed=3) for s in sources]
    plain_in = [torch.from_numpy(i.copy()).cuda() for i in imgs]
    for flags in (0, 1):
        plain_out = [torch.empty(fpng_amd.max_encoded_size(i.shape[1], i.shape[0], c) + 64, dtype=torch.uint8, device="cuda") for i in imgs]
        enc.submit(plain_in, plain_out, flags)
        t0 = enc.last_ticket
        flying = [st.submit(enc, flags) for st in sts]
        assert [f[0] for f in flying] == [t0 + 1, t0 + 2, t0 + 3]
        for st, fly in reversed(list(zip(sts, flying))):
            for img, png in zip(imgs, st.collect(enc, *fly)):
                _same(png, expected(img, flags), f"{_sid(st.src)} among four submissions, flags {flags}, {img.shape[1]}x{img.shape[0]}")
        for img, out, (size, _, status) in zip(imgs, plain_out, enc.wait(t0, len(imgs))):
            assert status == 0
            _same(bytes(out[:size].cpu().numpy()), expected(img, flags), f"plain among four submissions, flags {flags}")
