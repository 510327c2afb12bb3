"""The host side of the general decode tier (fpng_amd/csrc/png_decode_api.cpp) on the GPU (-m gpu): the IHDR and size limits, one
batch that mixes every kind of refusal with files of both tiers, the scratch groups together with the routing, and the rule that
a refused file's destination stays as it was.  Destinations are filled with 0xA5 and lie between guard bands; expectations are the
plain model's pixels (tests/unfilter_cases.py), the fpng path's own pixels, and the status table of include/fpng_amd.h."""
import os
import struct
import zlib

import numpy as np
import pytest

import png_cases as pc
import unfilter_cases as uc
from test_gpu_decode_png import GUARD, _fpng_files, _to_device, enc  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu
INVALID_ARG, DIMENSIONS_TOO_LARGE = 2, 6


def run(enc, files, desired, sizes, host=False, flags=0):
    """decode() of test_gpu_decode_png.py that keeps the destinations: -> [(status, channels_in_file, the destination's sizes[i] bytes
    after the call)]; every destination is 0xA5 before the call and the guard bands around each must still be"""
    import torch
    arena = torch.full((sum(sizes) + GUARD * (len(files) + 1),), 0xA5, dtype=torch.uint8, device="cuda")
    outs, at = [], GUARD
    for n in sizes:
        outs.append(arena[at:at + n])
        at += n + GUARD
    if host:
        res = enc.decode_batch_png([bytes(f) for f in files], desired, outs=outs, flags=flags)
    else:
        res = enc.decode_device_png(_to_device(files), desired, outs=outs, flags=flags)
    torch.cuda.synchronize()
    a = arena.cpu().numpy()
    out, at = [], 0
    for (st, _, chans), n in zip(res, sizes):
        assert (a[at:at + GUARD] == 0xA5).all(), f"guard in front of file {len(out)}"
        out.append((st, chans, a[at + GUARD:at + GUARD + n]))
        at += GUARD + n
    assert (a[at:at + GUARD] == 0xA5).all(), "guard behind the last file"
    return out


def header_only(w, h, color=0, stream=b"\x78\x01\x03"):
    """a valid header and a few IDAT bytes"""
    return pc.png(w, h, color, stream)


@pytest.mark.parametrize("form", ["device", "host"])
@pytest.mark.parametrize("desired", [3, 4])
def test_ihdr_limits(enc, form, desired):
    """2^24 a side and 2^30 pixels; every destination is one byte and stays as it was"""
    files = [header_only((1 << 24) + 1, 1), header_only(1, (1 << 24) + 1), header_only(32768, 32769)]
    want = [pc.BAD_DIMS] * 3
    if desired == 4:  # (2^32 bytes of pixels: no 32-bit size holds them)
        files.append(header_only(32768, 32768))
        want.append(DIMENSIONS_TOO_LARGE)
    got = run(enc, files, desired, [1] * len(files), host=form == "host")
    assert [st for st, _, _ in got] == want
    assert all(d.tolist() == [0xA5] for _, _, d in got)


@pytest.mark.parametrize("form", ["device", "host"])
def test_room_is_checked_before_anything_is_launched(enc, form):
    """32768 x 32768 at 3 channels passes the header and the 32-bit size; its one-byte destination does not hold it: the call fails,
    and the good file in front of it has not been decoded"""
    import torch
    import fpng_amd
    good = uc.predictor_cases()[0]
    files = [good.file, header_only(32768, 32768)]
    outs = [torch.full((good.w * good.h * 3,), 0xA5, dtype=torch.uint8, device="cuda"), torch.full((1,), 0xA5, dtype=torch.uint8, device="cuda")]
    with pytest.raises(fpng_amd.FpngAmdError):
        if form == "host":
            enc.decode_batch_png(files, 3, outs=outs)
        else:
            enc.decode_device_png(_to_device(files), 3, outs=outs)
    torch.cuda.synchronize()
    assert all(bool((t == 0xA5).all()) for t in outs)


@pytest.mark.parametrize("desired", [3, 4])
def test_widest_row_passes_the_header(enc, desired):
    """2^24 x 1 is inside the limits: the file goes to the kernels, its cut stream gives INVALID_IDAT, and no byte of its
    destination (which must hold the whole image: the room check) is touched"""
    stream = zlib.compress(bytes(1) + np.random.default_rng(1).integers(0, 256, 6000, dtype=np.uint8).tobytes(), 1)
    (st, _, dest), = run(enc, [header_only(1 << 24, 1, 0, stream[:len(stream) // 2])], desired, [(1 << 24) * desired])
    assert st == pc.INVALID_IDAT and (dest == 0xA5).all()


@pytest.mark.parametrize("form", ["device", "host"])
def test_file_size_limits(enc, form):
    """57 bytes: NOT_PNG whatever they hold; 58 bytes with a good header go on to the chunk walk, which gives the answer"""
    ihdr = header_only(1, 1)[:33]
    f57 = ihdr + pc.chunk(b"IDAT") + pc.chunk(b"IEND")
    f58_no_idat = ihdr + pc.chunk(b"tEXt", b"a") + pc.chunk(b"IEND")
    f58_idat = ihdr + pc.chunk(b"IDAT", b"\x78") + pc.chunk(b"IEND")
    assert [len(f) for f in (f57, f58_no_idat, f58_idat)] == [57, 58, 58]
    got = run(enc, [f57, f58_no_idat, f58_idat], 4, [4, 4, 4], host=form == "host")
    assert [st for st, _, _ in got] == [pc.NOT_PNG, pc.CHUNK_PARSING, pc.INVALID_IDAT]
    assert all((d == 0xA5).all() for _, _, d in got)


# ---- one mixed batch ----
class Entry:
    """file, the status it must give, its destination's size; pixels: the expected ones (numpy), or None for a refusal;
    untouched: the destination must stay 0xA5 (every refusal but the un-filter pass's own, which writes pixels before it answers)"""

    def __init__(self, name, file, status, size, pixels=None, untouched=True, general=False):
        self.name, self.file, self.status, self.size, self.pixels, self.untouched, self.general = name, file, status, size, pixels, untouched, general


def mixed_batch(enc, desired):
    damage = {n: (f, st) for n, f, st in pc.damage_cases()}
    fpng = _fpng_files(enc)
    out = [Entry("empty", b"", INVALID_ARG, 64)]
    ihdr = header_only(1, 1)[:33]
    out.append(Entry("57_bytes", ihdr + pc.chunk(b"IDAT") + pc.chunk(b"IEND"), pc.NOT_PNG, 64))
    for name in ("bad_signature", "depth16_color2", "adam7"):
        out.append(Entry(name, damage[name][0], damage[name][1], 20 * 12 * desired))
    assert [e.status for e in out[2:]] == [pc.NOT_PNG, pc.UNSUPPORTED, pc.UNSUPPORTED]
    section2 = [uc.predictor_cases()[2], uc.chain_cases()[7], [c for c in uc.shape_cases() if c.dims == (129, 65)][0],
                [c for c in uc.expansion_cases() if c.name == "trns_in_front_of_plte"][0]]
    refusal = [c for c in uc.refusal_cases() if c.name == "palette10_index_row64"][0]

    def model(c):
        return Entry(c.name, c.file, 0, c.w * c.h * desired, c.expected(desired), general=True)

    def fast(name, f):
        w, h = struct.unpack(">II", f[16:24])
        (st, px, _), = enc.decode_device(_to_device([f]), desired, [(w, h)])
        assert st == 0, name
        return Entry(name, f, 0, w * h * desired, px.cpu().numpy())

    out.append(fast(*fpng[0]))
    out.append(model(section2[0]))
    out.append(fast(*fpng[3]))
    name, f = fpng[4]  # the golden file the fpng path leaves UNDECIDED: the general tier's, judged by Pillow with its checksums repaired
    assert name == "first_pixel_match"
    exp = pc.expected(pc.repair_checksums(f), desired)
    out.append(Entry(name, f, 0, exp.size, exp, general=True))
    out += [model(c) for c in section2[1:]]
    # (a refusal inside the un-filter pass writes pixels before it answers: only its guard bands are asserted)
    out.append(Entry(refusal.name, refusal.file, pc.INVALID_IDAT, refusal.w * refusal.h * desired, untouched=False, general=True))
    return out


def run_mixed(enc, batch, desired, host=False, flags=0):
    got = run(enc, [e.file for e in batch], desired, [e.size for e in batch], host=host, flags=flags)
    for e, (st, _, dest) in zip(batch, got):  # every result at its own index
        assert st == e.status, (e.name, st, host, flags)
        if e.pixels is not None:
            assert np.array_equal(dest, e.pixels.reshape(-1)), (e.name, host, flags)
        elif e.untouched:
            assert (dest == 0xA5).all(), (e.name, host, flags)
    return got


@pytest.mark.parametrize("form", ["device", "host"])
@pytest.mark.parametrize("desired", [3, 4])
def test_mixed_batch(enc, form, desired):
    """null, short, foreign, unsupported, fpng-written, undecided and general-tier files in one call"""
    batch = mixed_batch(enc, desired)
    assert len(batch) == 13 and sum(e.pixels is not None for e in batch) == 7
    got = run_mixed(enc, batch, desired, host=form == "host")
    chans = {e.name: c for e, (_, c, _) in zip(batch, got)}
    assert chans["first_pixel_match"] == 4 and chans["trns_in_front_of_plte"] == 4 and chans["predictors_bpp3"] == 3


def _groups(needs, limit):
    """how many groups the batch's general-tier files make (include/fpng_amd.h: a file joins the group while the sum stays at or
    under the limit; a file that alone exceeds it is a group of its own)"""
    groups, room = 0, 0
    for need in needs:
        if not groups or room + need > limit:
            groups, room = groups + 1, 0
        room += need
    return groups


def _needs(batch, host):
    """the general tier's files in the order the call takes them: those routed there at once, then what the fpng path left.  Scanlines,
    and in the host form the file's bytes, each rounded up to 256"""
    order = [e for e in batch if e.general and e.name != "first_pixel_match"] + [e for e in batch if e.name == "first_pixel_match"]
    out = []
    for e in order:
        w, h = struct.unpack(">II", e.file[16:24])
        scan = h * (1 + w * pc.BPP[e.file[25]])
        out.append((scan + 255) // 256 * 256 + ((len(e.file) + 255) // 256 * 256 if host else 0))
    return out


@pytest.mark.parametrize("form", ["device", "host"])
def test_groups_and_routing_together(enc, form):
    """the mixed batch with every general-tier file a group of its own, and in three groups: statuses and pixels as in one group"""
    host = form == "host"
    batch = mixed_batch(enc, 4)
    needs = _needs(batch, host)
    assert len(needs) == 6 and _groups(needs, 1 << 30) == 1
    one = run_mixed(enc, batch, 4, host=host)
    three = next(limit for limit in range(max(needs), sum(needs), 256) if _groups(needs, limit) == 3)
    for limit, groups in ((256, 6), (three, 3)):
        assert _groups(needs, limit) == groups
        os.environ["FPNG_AMD_PNG_SCRATCH_LIMIT"] = str(limit)
        try:
            got = run_mixed(enc, batch, 4, host=host)
        finally:
            del os.environ["FPNG_AMD_PNG_SCRATCH_LIMIT"]
        for e, a, b in zip(batch, one, got):
            assert a[:2] == b[:2], (e.name, limit)
            if e.status == 0:
                assert np.array_equal(a[2], b[2]), (e.name, limit)


@pytest.mark.parametrize("form", ["device", "host"])
def test_general_only_on_the_mixed_batch(enc, form):
    """FPNG_AMD_PNG_GENERAL_ONLY: the fpng-written files give the fast path's pixels, every other entry its answer as before"""
    for desired in (3, 4):
        run_mixed(enc, mixed_batch(enc, desired), desired, host=form == "host", flags=1)
