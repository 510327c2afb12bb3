"""GPU decoder at the dimension limits (-m gpu): the decoder takes w, h <= 2^24 with w * h <= 2^30 (png_parse.h), and no other test
has a dimension above 24000.  Two groups of files, all through every destination -- packed (host and device files, 3 and 4
channels), bottom-up BGRA, planar, f16 planes, crops (uint8 and bf16) at the far corner and edges, and once with the checksums
verified:

  truthful  a dimension of 65535, the largest an fpng encoder can state (IHDR gets only the low 16 bits of each dimension, as in the
            reference): 256 column blocks in one segment, or 1366 segments of one block;
  patched   65536 and 2^24 in a dimension: files no encoder writes -- the oracle's file with IHDR corrected to the true dimensions
            (container_mutator.with_dimensions) -- but which the decoder accepts and runs its kernels on: a row of 2^26 bytes, 65536
            column blocks, or 349526 look-back segments in one column.

Content is test_widths_around_the_unfilter_kernels_wave_and_workgroup_edges' smooth generator (Deflate blocks, not stored ones).  The
judge (the reference's decoder) gives every file's status and confirms that the source pixels ARE what the file holds; the GPU's
pixels are then compared with the source on the device.  FPNG_AMD_DECODE_UNDECIDED is a failure here: no file has a match at a row's
first pixel, so it would mean that the look-back gave up or the synchronisation did not converge."""
import numpy as np
import pytest

import container_mutator as CM
from cpu_ref import oracle
from test_gpu_decode import _device_files, judge
from test_gpu_decode_crop import _decode_crop, _first_difference, _regions as _crop_regions, _sentinel as _crop_sentinel
from test_gpu_decode_float import CONSTS, _bits as _table_bits, _tables
from test_gpu_decode_layouts import SENTINEL
from test_gpu_decode_planar import KINDS

pytestmark = pytest.mark.gpu

BIG = 1 << 24
MARGIN = 4096
# (w, h, channels, flags of each file)
TRUTHFUL = [(65535, 3, 3, (0, 1)), (65535, 2, 4, (0, 1)), (3, 65535, 4, (0, 1)), (1, 65535, 3, (0, 1))]
PATCHED_SMALL = [(65536, 2, 4, (0, 1)), (1, 65536, 3, (0, 1))]
PATCHED_BIG = [(BIG, 2, 4, (0,)), (BIG, 2, 3, (1,)), (1, BIG, 4, (0,)), (2, BIG, 3, (1,))]
DESTS = ["packed", "ex", "planar", "float16", "crop_uint8", "crop_bfloat16", "verify"]


def smooth_image(w, h, c, rng):
    """(3 x + 2 y + 17 ch + {0, 1, 2}) & 255 as (h, w, c) uint8: one 4096-pixel period of the row term tiled (3 * 4096 = 0 mod 256),
    the row and noise terms added in wrapping uint8 arithmetic"""
    x, ch = np.meshgrid(np.arange(min(w, 4096)), np.arange(c), indexing="ij")
    period = ((3 * x + 17 * ch) & 255).astype(np.uint8)
    row = np.tile(period, ((w + 4095) // 4096, 1))[:w]
    img = rng.integers(0, 3, size=(h, w, c), dtype=np.uint8)
    img += row[None, :, :]
    img += (2 * np.arange(h) & 255).astype(np.uint8)[:, None, None]
    return img


class _File:
    def __init__(self, img, flags, patched):
        import torch
        h, w, c = img.shape
        self.w, self.h, self.c, self.flags, self.img = w, h, c, flags, img
        png = oracle().encode(img, w, h, c, flags)
        stated = (int.from_bytes(png[16:20], "big"), int.from_bytes(png[20:24], "big"))
        assert stated == (w & 0xFFFF, h & 0xFFFF)  # the low 16 bits, as the reference writes them
        assert patched == (stated != (w, h))
        self.png = CM.with_dimensions(png, w, h) if patched else png
        assert (self.png[60] & 6) != 0  # Deflate blocks
        self.status, px, jw, jh, jc = judge(self.png, c)
        assert self.status == 0 and (jw, jh, jc) == (w, h, c)
        assert np.array_equal(np.asarray(px)[: w * h * c], img.reshape(-1))  # the judge's pixels are the source's
        self.dev = torch.from_numpy(img).cuda()

    def want(self, d):
        """(h, w, d) on the device: the source at d channels, as the reference converts (alpha 255 added, or dropped)"""
        import torch
        if d == self.c:
            return self.dev
        if d < self.c:
            return self.dev[:, :, :d]
        return torch.cat([self.dev, torch.full_like(self.dev[:, :, :1], 255)], dim=2)

    def window(self, crop, d):
        """the crop's (h, w, d) pixels on the host"""
        x, y, w, h = crop
        px = self.img[y:y + h, x:x + w, :min(d, self.c)]
        return px if d <= self.c else np.concatenate([px, np.full_like(px[:, :, :1], 255)], axis=2)

    def crops(self):
        w, h = self.w, self.h
        out = [(max(w - 5, 0), max(h - 2, 0), min(w, 5), min(h, 2))]  # the far corner
        if h > w:
            out.append((0, h - 50, w, 50))  # every segment above publishes and writes nothing
        else:
            out += [(w - 300, 0, 300, h), (255, 0, 2, h)]  # the last column blocks; across a block border
        return out


@pytest.fixture(scope="module")
def enc(built_lib):
    import torch
    import fpng_amd
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    e = fpng_amd.Encoder(device=0)
    yield e
    e.close()


def _make(shapes, patched, seed):
    rng = np.random.default_rng(seed)
    return [_File(smooth_image(w, h, c, rng), fl, patched) for (w, h, c, flags) in shapes for fl in flags]


@pytest.fixture(scope="module")
def truthful():
    return _make(TRUTHFUL, False, 41)


@pytest.fixture(scope="module")
def patched_small():
    return _make(PATCHED_SMALL, True, 42)


@pytest.fixture(scope="module")
def patched_big():
    return _make(PATCHED_BIG, True, 43)


def _guarded(shape, dtype):
    """a sentinel-filled device tensor of `shape` between two sentinel-filled margins: (the whole buffer as bytes, the tensor)"""
    import torch
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    buf = torch.full((n + 2 * MARGIN,), SENTINEL, dtype=torch.uint8, device="cuda")
    return buf, buf[MARGIN:MARGIN + n].view(dtype).view(shape)


def _margins_kept(bufs):
    return all(bool((b[:MARGIN] == SENTINEL).all()) and bool((b[-MARGIN:] == SENTINEL).all()) for b in bufs)


def _ok(got, files, what):
    for i, ((st, _, cf), f) in enumerate(zip(got, files)):
        assert st == f.status == 0 and cf == f.c, (what, i, (f.w, f.h, f.c, f.flags), st, cf)


def _packed(enc, files, what="packed"):
    import torch
    dev = _device_files([f.png for f in files], shift=1)
    for d in (3, 4):
        for name, got in (("decode_batch", enc.decode_batch([f.png for f in files], d)),
                          ("decode_device", enc.decode_device(dev, d, [(f.w, f.h) for f in files]))):
            _ok(got, files, (what, name, d))
            for i, ((_, px, _), f) in enumerate(zip(got, files)):
                assert tuple(px.shape) == (f.h, f.w, d) and torch.equal(px, f.want(d)), (what, name, d, i, (f.w, f.h, f.c, f.flags))


def _ex(enc, files):
    import torch
    made = [_guarded((f.h, f.w, 4), torch.uint8) for f in files]
    got = enc.decode_device_ex(_device_files([f.png for f in files], shift=2), [t for _, t in made], order="bgra", bottom_up=True)
    _ok(got, files, "ex")
    for i, ((_, t), f) in enumerate(zip(made, files)):
        assert torch.equal(t, f.want(4)[:, :, [2, 1, 0, 3]].flip(0)), ("ex", i, (f.w, f.h, f.c, f.flags))
    assert _margins_kept([b for b, _ in made])


def _planar(enc, files):
    import torch
    made = [_guarded((3 + (i & 1), f.h, f.w), torch.uint8) for i, f in enumerate(files)]
    got = enc.decode_device_planar(_device_files([f.png for f in files], shift=3), [t for _, t in made])
    _ok(got, files, "planar")
    for i, ((_, t), f) in enumerate(zip(made, files)):
        assert torch.equal(t, f.want(3 + (i & 1)).permute(2, 0, 1)), ("planar", i, (f.w, f.h, f.c, f.flags))
    assert _margins_kept([b for b, _ in made])


def _float16(enc, files):
    import torch
    consts = CONSTS[1]
    tab = torch.from_numpy(_tables(consts, "float16").view(np.int16)).cuda()
    made = [_guarded((4 - (i & 1), f.h, f.w), torch.float16) for i, f in enumerate(files)]
    got = enc.decode_device_float(_device_files([f.png for f in files], shift=1), [t for _, t in made], scale=consts[0], bias=consts[1])
    _ok(got, files, "float16")
    for i, ((_, t), f) in enumerate(zip(made, files)):
        want = f.want(4 - (i & 1))
        for ch in range(want.shape[2]):
            exp = tab[ch].index_select(0, want[:, :, ch].reshape(-1).to(torch.int32)).view(f.h, f.w)
            assert torch.equal(t[ch].view(torch.int16), exp), ("float16", i, ch, (f.w, f.h, f.c, f.flags))
    assert _margins_kept([b for b, _ in made])


def _crop(enc, files, dtype):
    """every crop of every file in ONE call into ONE sentinel-filled buffer, compared whole"""
    batch = [(f, crop) for f in files for crop in f.crops()]
    crops = [crop for _, crop in batch]
    c = 3 if dtype == "uint8" else 4
    regs, total = _crop_regions(crops, c, [KINDS[k % len(KINDS)] for k in range(len(batch))])
    consts = CONSTS[0]
    dev = dict(zip(map(id, files), _device_files([f.png for f in files], shift=1)))  # (one upload per file, shared by its crops)
    got, host, _ = _decode_crop(enc, [f.png for f, _ in batch], crops, regs, total, dtype, True, consts=consts, dev=[dev[id(f)] for f, _ in batch])
    _ok(got, [f for f, _ in batch], "crop " + dtype)
    tab = None if dtype == "uint8" else _tables(consts, dtype)
    exp = np.full(total, _crop_sentinel(dtype), dtype=host.dtype)
    for r, (f, crop) in zip(regs, batch):
        px = f.window(crop, c)
        r.put(exp, px if tab is None else _table_bits(px, tab))
    assert _first_difference(host, exp, regs) is None, (dtype, _first_difference(host, exp, regs), crops)


def _verify(enc, files):
    enc.set_decode_verify(3)
    try:
        _packed(enc, files, "verify")
    finally:
        enc.set_decode_verify(0)


def _run(enc, files, dest):
    {"packed": _packed, "ex": _ex, "planar": _planar, "float16": _float16, "verify": _verify,
     "crop_uint8": lambda e, f: _crop(e, f, "uint8"), "crop_bfloat16": lambda e, f: _crop(e, f, "bfloat16")}[dest](enc, files)


@pytest.mark.parametrize("dest", DESTS)
def test_truthful_files(enc, truthful, dest):
    """65535 x 3 x 3, 65535 x 2 x 4, 3 x 65535 x 4 and 1 x 65535 x 3, 1-pass and 2-pass, as the encoder wrote them: one batch"""
    _run(enc, truthful, dest)


@pytest.mark.parametrize("dest", DESTS)
def test_patched_files_just_past_16_bits(enc, patched_small, dest):
    """65536 x 2 x 4 and 1 x 65536 x 3, 1-pass and 2-pass, header corrected: one batch"""
    _run(enc, patched_small, dest)


@pytest.mark.parametrize("dest", DESTS)
def test_patched_files_at_the_largest_dimension(enc, patched_big, dest):
    """2^24 x 2 x 4, 2^24 x 2 x 3, 1 x 2^24 x 4 and 2 x 2^24 x 3 (1-pass and 2-pass alternate), header corrected: one batch -- rows of
    2^26 bytes in 65536 column blocks (the wide crops start at column block 65534), and 349526 look-back segments in one column"""
    _run(enc, patched_big, dest)


def test_streamed_host_decode_at_the_largest_dimension(enc, patched_big):
    """decode_host on 2^24 x 2 x 4 and 1 x 2^24 x 4: an IDAT of more than 8 MiB goes through the streamed form (offsets by range,
    un-filter launches at a later item0)"""
    for f in (patched_big[0], patched_big[2]):
        assert f.c == 4 and len(f.png) > (8 << 20)
        st, px, cf = enc.decode_host(f.png, 4)
        assert st == f.status == 0 and cf == 4, (f.w, f.h, st)
        assert px.shape == f.img.shape and np.array_equal(px, f.img), (f.w, f.h)


def test_one_column_of_2_to_the_24_next_to_small_files(enc, patched_big):
    """one decode_device call with 1 x 2^24 x 4 between four 64 x 97 files: an un-filter plan with pieces of 349526 segments and of 3"""
    import torch
    rng = np.random.default_rng(44)
    small = [smooth_image(64, 97, 3 + (k & 1), rng) for k in range(4)]
    spng = [oracle().encode(im, 64, 97, im.shape[2], k & 1) for k, im in enumerate(small)]
    f = patched_big[2]
    assert (f.w, f.h) == (1, BIG)
    pngs = spng[:2] + [f.png] + spng[2:]
    got = enc.decode_device(_device_files(pngs, shift=1), 4, [(64, 97)] * 2 + [(1, BIG)] + [(64, 97)] * 2)
    for i, (png, (st, px, cf)) in enumerate(zip(pngs, got)):
        if i == 2:
            assert st == 0 and cf == 4 and torch.equal(px, f.want(4)), i
        else:
            cst, cpx, w, h, c = judge(png, 4)
            assert st == cst == 0 and cf == c and np.array_equal(px.cpu().numpy().reshape(-1), np.asarray(cpx)[: w * h * 4]), i
