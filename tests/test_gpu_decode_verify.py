"""The optional check of a file's IDAT CRC-32 and Adler-32 by the GPU decoder (-m gpu; fpng_amd_encoder_set_decode_verify:
dec_crc_kernel, the verify forms of dec_unfilter_kernel, dec_stored_adler_kernel, dec_verify_kernel).

Files are this project's encoder's, from synth_image content.  Python's zlib is the judge of every damaged file
(tests/verify_files.py); the decoder's own answer is only used for verify 0, to show that the damage passes by default, and to
compare the pixels of clean files with and without the check.  Every GPU step runs once; the damaged files are valid streams with
wrong checksums, which the decoder takes with status 0 by default."""
import os
import struct
import zlib

import numpy as np
import pytest

import verify_files as vf
from test_gpu_decode import UNDECIDED, _device_files

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0xA5
SMALL = [(1, 1), (5, 3), (257, 49)]
KINDS = ("noise", "solid", "grad", "blocks")


@pytest.fixture(scope="module")
def enc(built_lib):
    import torch
    import fpng_amd
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    e = fpng_amd.Encoder(device=0)
    yield e
    e.set_decode_verify(0)
    e.close()


def _encode(enc, img, flags):
    import torch
    (png,), _ = enc.encode_tensors([torch.from_numpy(np.ascontiguousarray(img)).cuda()], flags)
    return bytes(png)


def _dims(png):
    return struct.unpack(">II", bytes(png[16:24]))


@pytest.fixture(scope="module")
def clean(enc):
    """[(name, file)]: flags 0, 1, 2 x 3 and 4 channels x the small sizes, 1023 x 97 RGB and 2048 x 2048, the four contents in turn"""
    import fpng_amd
    out, k = [], 0
    for (w, h) in SMALL + [(1023, 97), (2048, 2048)]:
        for c in (3, 4):
            if (w, h) == (1023, 97) and c == 4:
                continue
            for fl in (0, 1, 2):
                kind = KINDS[k % 4]
                k += 1
                png = _encode(enc, fpng_amd.synth_image(kind, w, h, c, seed=k), fl)
                assert not vf.crc_is_bad(png) and not vf.adler_is_bad(png), (w, h, c, fl, kind)
                out.append((f"{kind}_{w}x{h}x{c}_f{fl}", png))
    return out


def _statuses(got):
    return [st for st, _, _ in got]


def _host(t):
    return t.cpu().numpy()


def _all_destinations(enc, pngs):
    """every destination of the batch calls -> {name: (statuses, [pixel bytes as numpy])}"""
    import torch
    dims = [_dims(p) for p in pngs]
    dev = _device_files(pngs, shift=1)
    res = {}
    for d in (3, 4):
        got = enc.decode_batch(pngs, d)
        res[f"host_packed{d}"] = (_statuses(got), [_host(px) for _, px, _ in got])
        got = enc.decode_device(dev, d, dims)
        res[f"device_packed{d}"] = (_statuses(got), [_host(px) for _, px, _ in got])
    # BGRA, a padded pitch, bottom-up; planes (3 and 4) with a padded pitch and a gap between the planes
    for device in (False, True):
        bufs = [torch.full((h * (4 * w + 64) + 128,), SENTINEL, dtype=torch.uint8, device="cuda") for (w, h) in dims]
        views = [b.as_strided((h, w, 4), (4 * w + 64, 4, 1), 64) for b, (w, h) in zip(bufs, dims)]
        got = (enc.decode_device_ex if device else enc.decode_batch_ex)(dev if device else pngs, views, "bgra", True)
        torch.cuda.synchronize()
        res[f"ex_{device}"] = (_statuses(got), [_host(b) for b in bufs])
        for planes in (3, 4):
            bufs = [torch.full((planes * (h * (w + 32) + 96) + 64,), SENTINEL, dtype=torch.uint8, device="cuda") for (w, h) in dims]
            views = [b.as_strided((planes, h, w), (h * (w + 32) + 96, w + 32, 1), 32) for b, (w, h) in zip(bufs, dims)]
            got = (enc.decode_device_planar if device else enc.decode_batch_planar)(dev if device else pngs, views)
            torch.cuda.synchronize()
            res[f"planar{planes}_{device}"] = (_statuses(got), [_host(b) for b in bufs])
    return res


def test_clean_files_every_destination(enc, clean):
    """verify 3: status 0 and the bytes of verify 0 -- pixels, and every sentinel byte of pitch padding and between the planes (the
    written-extent promise) -- through packed 3 and 4, BGRA bottom-up with a padded pitch, three and four planes, host and device files"""
    pngs = [p for _, p in clean]
    enc.set_decode_verify(0)
    base = _all_destinations(enc, pngs)
    enc.set_decode_verify(3)
    try:
        got = _all_destinations(enc, pngs)
    finally:
        enc.set_decode_verify(0)
    assert set(base) == set(got)
    for name in base:
        assert base[name][0] == [0] * len(pngs), name
        assert got[name][0] == [0] * len(pngs), (name, [(clean[i][0], s) for i, s in enumerate(got[name][0]) if s])
        for i, (a, b) in enumerate(zip(base[name][1], got[name][1])):
            assert np.array_equal(a, b), (name, clean[i][0])
    # (the sentinel bytes are there at all: the comparison above is not of two fully written buffers)
    assert (base["ex_True"][1][-1] == SENTINEL).sum() >= 64 * 2048 and (base["planar4_False"][1][-1] == SENTINEL).sum() >= 32 * 2048


def test_decode_host_and_8k_frames(enc):
    """fpng_amd_decode_host on one 7680 x 4320 RGBA grad (58 MB of IDAT: the path that streams by default) and on a solid frame
    (long matches, resume points): verify 3 gives status 0 and the pixels of verify 0; so does the device entry point.  One literal
    of the solid frame changed, in a late segment, with a stale Adler-32: 0 / 0 / 66 / 66 for verify 0 .. 3 (CRC recomputed)."""
    import fpng_amd
    from test_decode_model import emul
    rng = np.random.default_rng(7)
    w, h = 7680, 4320
    for kind in ("grad", "solid"):
        img = fpng_amd.synth_image(kind, w, h, 4, seed=3)
        png = _encode(enc, img, 0)
        assert not vf.crc_is_bad(png) and not vf.adler_is_bad(png)
        enc.set_decode_verify(0)
        st0, px0, _ = enc.decode_host(png, 4)
        enc.set_decode_verify(3)
        try:
            st3, px3, _ = enc.decode_host(png, 4)
            (std, pxd, _), = enc.decode_device(_device_files([png], shift=3), 4, [(w, h)])
        finally:
            enc.set_decode_verify(0)
        assert (st0, st3, std) == (0, 0, 0), kind
        assert np.array_equal(px0, px3) and np.array_equal(px0.reshape(-1), img.reshape(-1)), kind
        assert np.array_equal(_host(pxd).reshape(-1), img.reshape(-1)), kind
        del px0, px3, pxd
        if kind == "solid":
            made = vf.edit_literal_large(png, emul(), 4000, 0, 4 * w, rng)
            assert made is not None
            stale, _ = made
            assert vf.adler_is_bad(stale) and not vf.crc_is_bad(stale)
            sts = []
            for knob in (0, 1, 2, 3):
                enc.set_decode_verify(knob)
                try:
                    sts.append(enc.decode_host(stale, 4)[0])
                finally:
                    enc.set_decode_verify(0)
            assert sts == [vf.expected_status(stale, k) for k in (0, 1, 2, 3)] == [0, 0, 66, 66]


def _damaged(enc):
    """[(name, file)]: the single-literal edit in the first tile, the last tile, and a tile of a later segment and a later column
    block (2048 x 2048 RGBA: 43 segments x 8 column blocks; 1023 x 97 RGB: 3 x 4, rows that end inside a dword), each with a stale
    Adler-32, CRC recomputed or not; the stored-byte edit at such places; a flipped bit of the CRC word"""
    import fpng_amd
    from test_decode_model import emul
    from token_mutator import LargeStream
    rng = np.random.default_rng(11)
    out = []
    for (w, h, c, fl) in [(2048, 2048, 4, 0), (1023, 97, 3, 1), (257, 49, 4, 0)]:
        png = _encode(enc, fpng_amd.synth_image("grad", w, h, c, seed=9), fl)
        assert vf.plan(png)[1] == 0
        s = LargeStream(png, vf.plan, emul())
        bpl = w * c
        places = {"first": (0, 0, min(bpl, 1024)), "last": (h - 1, max(0, bpl - min(bpl, 1024) // 2), bpl), "later": (h - h // 3, bpl // 2, bpl // 2 + min(bpl // 2, 512))}
        for tag, (row, lo, hi) in places.items():
            made = vf.edit_literal_large(png, None, row, lo, hi, rng, stream=s)
            assert made is not None, (w, h, tag)
            out += [(f"lit_{w}x{h}_{tag}", made[0]), (f"lit_nocrc_{w}x{h}_{tag}", made[1])]
        out.append((f"crcbit_{w}x{h}", vf.flip_crc_bit(png, int(rng.integers(0, 32)))))
    for (w, h, c) in [(2048, 2048, 3), (257, 49, 4), (5, 3, 3)]:
        png = _encode(enc, fpng_amd.synth_image("noise", w, h, c, seed=5), 2)
        assert vf.plan(png)[1] == 1
        for tag, (y, xb) in {"first": (0, 0), "last": (h - 1, w * c - 1), "later": (h - h // 3, (w * c) // 2)}.items():
            out += [(f"stored_{w}x{h}_{tag}", vf.edit_stored_byte(png, w, h, c, y, xb)), (f"stored_nocrc_{w}x{h}_{tag}", vf.edit_stored_byte(png, w, h, c, y, xb, fix_crc=False))]
        out.append((f"crcbit_stored_{w}x{h}", vf.flip_crc_bit(png, int(rng.integers(0, 32)))))
    return out


@pytest.fixture(scope="module")
def damaged(enc):
    return _damaged(enc)


@pytest.mark.parametrize("device", [False, True])
def test_damaged_files_get_what_zlib_says(enc, damaged, device):
    pngs = [p for _, p in damaged]
    dims = [_dims(p) for p in pngs]
    files = _device_files(pngs, shift=2) if device else pngs
    got = {}
    for knob in (0, 1, 2, 3):
        enc.set_decode_verify(knob)
        try:
            got[knob] = _statuses(enc.decode_device(files, 4, dims) if device else enc.decode_batch(files, 4))
        finally:
            enc.set_decode_verify(0)
    seen = set()
    for i, (name, png) in enumerate(damaged):
        crc_bad, adler_bad = vf.crc_is_bad(png), vf.adler_is_bad(png)
        assert (crc_bad, adler_bad) == (("nocrc" in name) or name.startswith("crcbit"), not name.startswith("crcbit")), name  # the cases are what they claim
        assert got[0][i] == 0, name  # the premise: the damage passes by default
        for knob in (1, 2, 3):
            assert got[knob][i] == vf.expected_status(png, knob), (name, knob, got[knob][i])
        if adler_bad:  # a one-byte change always moves s1: every such file is caught, no allowance
            assert got[2][i] == 66 and got[3][i] == (65 if crc_bad else 66) and got[1][i] == (65 if crc_bad else 0), name
        seen.add((crc_bad, adler_bad))
    assert seen == {(False, True), (True, True), (True, False)}


def test_one_damaged_file_among_sixteen(enc, clean, damaged):
    """only the damaged file's status changes; every other file's pixels are those of the unverified decode"""
    pngs = [p for n, p in clean if "2048" not in n][:15]
    bad = dict(damaged)["lit_1023x97_later"]
    pngs.insert(6, bad)
    dims = [_dims(p) for p in pngs]
    files = _device_files(pngs, shift=1)
    enc.set_decode_verify(0)
    base = enc.decode_device(files, 4, dims)
    base_px = [_host(px) for _, px, _ in base]
    enc.set_decode_verify(3)
    try:
        got = enc.decode_device(files, 4, dims)
    finally:
        enc.set_decode_verify(0)
    assert len(pngs) == 16 and _statuses(base) == [0] * 16
    assert _statuses(got) == [66 if i == 6 else 0 for i in range(16)]
    for i, (st, px, _) in enumerate(got):
        if i != 6:
            assert np.array_equal(_host(px), base_px[i]), i


def test_undecided_and_failing_files_keep_their_status(enc, clean):
    """verify 3 changes nothing about a file whose status is not 0 today: FPNG_AMD_DECODE_UNDECIDED (a match at a row's first pixel;
    every compressed file with FPNG_AMD_DECODE_MAX_ROUNDS=0) and the reference's failure codes of container_mutator, token_mutator
    and header_mutator files.  Files of those sets that decode today get zlib's verdict (token_mutator writes no Adler-32)."""
    from test_gpu_decode_layouts import _damaged_files, _header_dims
    from test_dropin_decode import other_tables
    golden = open(os.path.join(ROOT, "tests", "golden", "first_pixel_match.png"), "rb").read()
    pngs = [golden] + _damaged_files() + [f for _, _, f in other_tables(np.random.default_rng(99), 12)] + [p for n, p in clean if "257x49" in n]
    dims = [_header_dims(p) for p in pngs]
    for device in (False, True):
        files = _device_files(pngs, shift=1) if device else pngs
        for forced in (False, True):
            if forced:
                os.environ["FPNG_AMD_DECODE_MAX_ROUNDS"] = "0"
            try:
                enc.set_decode_verify(0)
                base = _statuses(enc.decode_device(files, 4, dims) if device else enc.decode_batch(files, 4))
                enc.set_decode_verify(3)
                got = _statuses(enc.decode_device(files, 4, dims) if device else enc.decode_batch(files, 4))
            finally:
                enc.set_decode_verify(0)
                if forced:
                    del os.environ["FPNG_AMD_DECODE_MAX_ROUNDS"]
            assert base[0] == UNDECIDED and any(s not in (0, UNDECIDED) for s in base)
            if forced:
                assert base.count(UNDECIDED) > 5
            judged = 0
            for i, (b, g) in enumerate(zip(base, got)):
                if b:
                    assert g == b, (device, forced, i, b, g)
                    continue
                if vf.crc_is_bad(pngs[i]):  # (zlib.crc32 has a verdict on every file, and 65 goes first)
                    want = 65
                else:
                    try:
                        want = vf.expected_status(pngs[i], 3)
                    except (AssertionError, zlib.error):
                        # an edited stream that zlib reads differently from fpng's decoders: no verdict on the Adler-32, but
                        # the CRC is right
                        assert g in (0, 66), (device, forced, i, g)
                        continue
                judged += 1
                assert g == want, (device, forced, i, b, g, want)
            assert judged >= 10


def test_setting_is_sticky_until_cleared(enc, damaged):
    bad = dict(damaged)["lit_257x49_first"]
    assert enc.decode_verify == 0
    enc.set_decode_verify(2)
    try:
        assert enc.decode_verify == 2
        assert _statuses(enc.decode_batch([bad], 4)) == [66]
        assert _statuses(enc.decode_batch([bad], 3)) == [66]  # (every later call)
        assert enc.decode_host(bad, 4)[0] == 66
    finally:
        enc.set_decode_verify(0)
    assert _statuses(enc.decode_batch([bad], 4)) == [0] and enc.decode_host(bad, 4)[0] == 0
    assert enc.lib.fpng_amd_encoder_set_decode_verify(enc.h, 4) == -1 and enc.decode_verify == 0


def test_written_extent_with_a_damaged_file(enc, damaged):
    """verify 3 and status 66 / 65: sentinel bytes in the pitch padding and between the planes stay in place"""
    import torch
    d = dict(damaged)
    pngs = [d["lit_1023x97_last"], d["stored_nocrc_257x49_later"], d["lit_2048x2048_first"]]
    dims = [_dims(p) for p in pngs]
    enc.set_decode_verify(3)
    try:
        for device in (False, True):
            files = _device_files(pngs, shift=1) if device else pngs
            bufs = [torch.full((h * (4 * w + 64) + 128,), SENTINEL, dtype=torch.uint8, device="cuda") for (w, h) in dims]
            views = [b.as_strided((h, w, 4), (4 * w + 64, 4, 1), 64) for b, (w, h) in zip(bufs, dims)]
            got = (enc.decode_device_ex if device else enc.decode_batch_ex)(files, views, "bgra", True)
            torch.cuda.synchronize()
            assert _statuses(got) == [66, 65, 66]
            for b, (w, h) in zip(bufs, dims):
                hb = _host(b)
                assert np.all(hb[:64] == SENTINEL) and np.all(hb[64 + (h - 1) * (4 * w + 64) + 4 * w:] == SENTINEL)
                assert np.all(hb[64:64 + h * (4 * w + 64)].reshape(h, 4 * w + 64)[:-1, 4 * w:] == SENTINEL)
            bufs = [torch.full((3 * (h * (w + 32) + 96) + 64,), SENTINEL, dtype=torch.uint8, device="cuda") for (w, h) in dims]
            views = [b.as_strided((3, h, w), (h * (w + 32) + 96, w + 32, 1), 32) for b, (w, h) in zip(bufs, dims)]
            got = (enc.decode_device_planar if device else enc.decode_batch_planar)(files, views)
            torch.cuda.synchronize()
            assert _statuses(got) == [66, 65, 66]
            for b, (w, h) in zip(bufs, dims):
                hb = _host(b)
                mask = np.ones(hb.size, dtype=bool)
                for p in range(3):
                    for y in range(h):
                        o = 32 + p * (h * (w + 32) + 96) + y * (w + 32)
                        mask[o:o + w] = False
                assert np.all(hb[mask] == SENTINEL)
    finally:
        enc.set_decode_verify(0)
