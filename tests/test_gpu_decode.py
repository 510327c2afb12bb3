"""GPU batch decoder of fpng-written files (-m gpu; fpng_amd_decode_batch / fpng_amd_decode_batch_device,
fpng_amd/csrc/decode.hip): pixels and status codes of the REFERENCE's decoder (oracle/_ref, a prebuilt file on the GPU box; without
it the drop-in's CPU decoder, itself checked against the reference's by tests/test_dropin_decode.py), also on damaged files;
FPNG_AMD_DECODE_UNDECIDED (= use the CPU decoder) is allowed only where the judge does not succeed either ... or, for valid
files, never in this suite unless a test asks for it."""
import hashlib
import os

import numpy as np
import pytest

import dropin
import real_image
from cpu_ref import ROOT, fuzz_image, have_ref, oracle, ref

pytestmark = pytest.mark.gpu
UNDECIDED = 64


def judge(png, desired):
    """(status, pixels, w, h, c) of the reference's decoder; without its build: the drop-in's CPU tier."""
    if have_ref():
        return ref().decode(png, desired)
    os.environ["FPNG_AMD_DECODE_CPU"] = "1"
    try:
        return dropin.decode(png, desired)
    finally:
        del os.environ["FPNG_AMD_DECODE_CPU"]


@pytest.fixture(scope="module")
def enc(built_lib):
    import torch
    import fpng_amd
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    e = fpng_amd.Encoder(device=0)
    yield e
    e.close()


def _device_files(pngs, shift=0):
    """the files in device memory, each at an address that is `shift` bytes (mod 4) off a dword boundary"""
    import torch
    out = []
    for k, p in enumerate(pngs):
        b = torch.zeros(len(p) + 8, dtype=torch.uint8, device="cuda")
        o = (shift + k) & 3 if shift else 0
        if len(p):
            b[o:o + len(p)] = torch.frombuffer(bytearray(p), dtype=torch.uint8).cuda()
        out.append(b[o:o + len(p)])
    return out


def _check(enc, pngs, desired, device=False, allow_undecided=False):
    """host-resident files through fpng_amd_decode_batch, or device-resident ones through fpng_amd_decode_batch_device"""
    import struct
    if device:
        dims = []
        for p in pngs:
            w, h = struct.unpack(">II", bytes(p[16:24])) if len(p) >= 24 else (0, 0)
            dims.append((w, h) if 0 < w <= (1 << 24) and 0 < h <= (1 << 24) and w * h <= (1 << 28) else (0, 0))
        got = enc.decode_device(_device_files(pngs, shift=1), desired, dims)
    else:
        got = enc.decode_batch(pngs, desired)
    n_ok = n_bad = n_left = 0
    for i, (png, (st, px, cf)) in enumerate(zip(pngs, got)):
        cst, cpx, w, h, c = judge(png, desired) if len(png) else (2, None, 0, 0, 0)
        if st == UNDECIDED and allow_undecided:
            assert cst != 0, i
            continue
        if st == UNDECIDED and cst == 0 and len(pngs) >= 100:
            # "the CPU decoder's": the one documented case with a file the reference takes is a match at a row's first pixel
            # (decode_core.h, walk_emit) -- no fpng encoder writes one, damage can.  What the drop-in then answers is checked.
            os.environ["FPNG_AMD_DECODE_CPU"] = "1"
            try:
                dst, dpx, *_ = dropin.decode(png, desired)
            finally:
                del os.environ["FPNG_AMD_DECODE_CPU"]
            assert dst == 0 and np.array_equal(np.asarray(dpx)[: w * h * desired], np.asarray(cpx)[: w * h * desired]), i
            n_left = n_left + 1
            assert n_left <= max(1, len(pngs) // 100), "too many files left to the CPU decoder"
            continue
        assert st == cst, (i, st, cst, len(png))
        if st == 0:
            assert cf == c and tuple(px.shape) == (h, w, desired)
            assert np.array_equal(px.cpu().numpy().reshape(-1), np.asarray(cpx)[: w * h * desired]), i
            n_ok += 1
        else:
            n_bad += 1
    return n_ok, n_bad


@pytest.mark.parametrize("desired", [3, 4])
def test_small_images_every_mode(enc, desired):
    """The fuzz recipe's images (runs, vertical copies, noise; ~40 % end up as stored blocks) encoded 1-pass, 2-pass and stored,
    decoded as one batch, to 3 and to 4 channels."""
    rng = np.random.default_rng(11)
    pngs = []
    for _ in range(150):
        img, w, h, c = fuzz_image(rng)
        for fl in (0, 1, 2):
            pngs.append(oracle().encode(img, w, h, c, fl))
    _check(enc, pngs, desired)
    _check(enc, pngs[:150], desired, device=True)


def test_a_descriptor_built_once_decodes_again_and_again(enc):
    """Encoder.make_decode_batch(): the C call's arrays filled once (what a C caller does anyway; bench.py's decode steps), the call
    repeated on them -- the same pixels every time, also after the output buffers were overwritten in between."""
    import torch
    rng = np.random.default_rng(12)
    pngs, frames = [], []
    for k in range(40):
        img, w, h, c = fuzz_image(rng)
        pngs.append(oracle().encode(img, w, h, c, k % 3))
        frames.append((w, h, c))
    dev = _device_files(pngs, shift=1)
    db = enc.make_decode_batch(dev, 4, [(w, h) for w, h, _ in frames])
    first = [(st, px.clone() if px is not None else None, cf) for st, px, cf in enc.decode_device(db)]
    for t in db.outs:
        t.fill_(0x5A)
    assert enc.decode_device(db, results=False) is db
    assert list(db.statuses()) == [st for st, _, _ in first]
    for i, ((st, px, cf), (st2, px2, cf2)) in enumerate(zip(first, db.results())):
        cst, cpx, w, h, c = judge(pngs[i], 4)
        assert st == st2 == cst, i
        if st == 0:
            assert cf == cf2 == c and torch.equal(px, px2), i
            assert np.array_equal(px2.cpu().numpy().reshape(-1), np.asarray(cpx)[: w * h * 4]), i


@pytest.mark.parametrize("desired", [3, 4])
def test_widths_around_the_unfilter_kernels_wave_and_workgroup_edges(enc, desired):
    """dec_unfilter_kernel writes 3 -> 4 and 4 -> 3 channels with gathers inside a wave (64 pixels) and takes 256 pixels or 256
    dword columns per workgroup; a segment has 48 rows.  Widths on both sides of those edges, heights with a short last segment,
    every channel combination, host- and device-resident (the latter at odd addresses)."""
    rng = np.random.default_rng(5)
    pngs = []
    for w in (1, 2, 5, 63, 64, 65, 85, 86, 191, 192, 193, 255, 256, 257, 341, 342, 343, 1023, 1024, 1025, 1367):
        for c in (3, 4):
            h = int(rng.integers(1, 110))
            y, x, ch = np.meshgrid(np.arange(h), np.arange(w), np.arange(c), indexing="ij")
            img = ((x * 3 + y * 2 + ch * 17 + rng.integers(0, 3, size=(h, w, c))) & 255).astype(np.uint8)  # (smooth: not stored blocks)
            pngs.append(oracle().encode(img, w, h, c, int(rng.integers(0, 2))))
    assert sum((p[60] & 6) != 0 for p in pngs) > len(pngs) * 3 // 4  # Deflate blocks, not stored ones
    _check(enc, pngs, desired)
    _check(enc, pngs, desired, device=True)


@pytest.mark.parametrize("desired", [3, 4])
def test_flat_rows_long_matches_and_resume_points(enc, desired):
    """Round 6's pass that writes: long matches are marked and filled a lane per pixel, a subsequence that puts out 2 KB and more leaves
    every window a resume point, long matches between literals have a step of their own.  Flat rows (one subsequence covers several
    windows of 256 pixels), flat rows with a few literal pixels in them at places that fall on window and wave edges, rows whose runs end
    in matches of two pixels, 3- and 4-channel, 1- and 2-pass, widths around the column blocks -- against the judge's pixels."""
    rng = np.random.default_rng(23)
    pngs = []
    for c in (3, 4):
        for w in (255, 256, 257, 700, 1024, 1031, 3000):
            h = int(rng.integers(50, 120))
            base = rng.integers(0, 256, size=(c,), dtype=np.uint8)
            img = np.broadcast_to(base, (h, w, c)).copy()
            img += (np.arange(h, dtype=np.uint8) * 3)[:, None, None]  # (a ramp down the rows: the Up filter leaves constant rows)
            kind = int(rng.integers(0, 4))
            if kind == 1:  # literal pixels on the edges of windows / waves
                for x in (0, 63, 64, 255, 256, 257, 511, 512, w - 1):
                    if x < w:
                        img[::3, x] = rng.integers(0, 256, size=(c,), dtype=np.uint8)
            elif kind == 2:  # runs of two pixels between literals
                img[:, ::3] = rng.integers(0, 256, size=(h, (w + 2) // 3, c), dtype=np.uint8)
            elif kind == 3:  # tiles: runs that end at block edges (matches with extra bits)
                img[:, :, 0] += ((np.arange(w) // 37) * 11).astype(np.uint8)[None, :]
            for fl in (0, 1):
                pngs.append(oracle().encode(np.ascontiguousarray(img), w, h, c, fl))
    assert sum((p[60] & 6) != 0 for p in pngs) > len(pngs) * 3 // 4  # Deflate blocks, not stored ones
    _check(enc, pngs, desired)
    _check(enc, pngs, desired, device=True)


def test_natural_image_and_synthetic_frames(enc):
    import torch
    import fpng_amd
    imgs = real_image.variants(real_image.rgb_pixels(dropin.decode))
    ts = [torch.from_numpy(imgs[k]).cuda() for k in ("rgb", "rgba_ga", "rgb_t4")]
    ts += [torch.from_numpy(fpng_amd.synth_image(kind, 3840, 2160, 4)).cuda() for kind in ("grad", "blocks", "noise", "solid")]
    for flags in (0, 1):
        pngs, _ = enc.encode_tensors(ts, flags)
        got = enc.decode_batch(pngs, 4)
        for t, (st, px, cf) in zip(ts, got):
            assert st == 0 and cf == t.shape[2]
            want = t if t.shape[2] == 4 else torch.cat([t, torch.full_like(t[:, :, :1], 255)], dim=2)
            assert torch.equal(px, want)
        got3 = enc.decode_batch(pngs[:3], 3)
        for t, (st, px, cf) in zip(ts[:3], got3):
            assert st == 0 and torch.equal(px, t[:, :, :3])


def test_groups_of_files_and_a_stream_that_needs_many_rounds(enc):
    """A batch of more than 8 MB of PNG goes through the GPU in up to four groups of files (upload of one overlapped with the
    decode of another).  A gradient WITHOUT noise (seed 0: the generator's xorshift stays 0) is a periodic token stream in which
    a decode started at a wrong bit stays out of step for dozens of subsequences: its group takes the extra-rounds path and is
    redone; stored files and small files share the groups."""
    import torch
    import fpng_amd
    ts = [torch.from_numpy(fpng_amd.synth_image("grad", 3840, 2160, 4, seed=sd)).cuda() for sd in (0, 5, 0, 6)]
    ts += [torch.from_numpy(fpng_amd.synth_image("noise", 1920, 1080, 3)).cuda(), torch.from_numpy(fpng_amd.synth_image("blocks", 1000, 700, 4)).cuda()]
    ts += [torch.from_numpy(fpng_amd.synth_image("grad", 640, 360, 3, seed=sd)).cuda() for sd in range(6)]
    for flags in (0, 1):
        pngs, _ = enc.encode_tensors(ts, flags)
        assert sum(len(p) for p in pngs) > (8 << 20)
        for desired in (4, 3):
            got = enc.decode_batch(pngs, desired)
            for t, (st, px, cf) in zip(ts, got):
                assert st == 0 and cf == t.shape[2]
                want = t[:, :, :desired] if t.shape[2] >= desired else torch.cat([t, torch.full_like(t[:, :, :1], 255)], dim=2)
                assert torch.equal(px, want)


def test_periodic_streams(enc):
    """Content whose token stream repeats itself (stripes on a vertical ramp, tiles: tests/test_decode_model.py has the CPU side):
    wrongly started decoders never fall into step, the candidate lists of dec_sync_kernel and dec_chain_kernel settle such files
    without walking through them subsequence by subsequence.  Pixels and status of the reference's decoder, host- and
    device-resident, whole and damaged; and a large striped frame must not take much longer than a gradient of its size."""
    import time
    import torch
    from test_decode_model import _damage, periodic_images
    rng = np.random.default_rng(17)
    pngs = []
    for name, img, w, h, c in periodic_images():
        for flags in (0, 1):
            png = oracle().encode(img, w, h, c, flags)
            pngs.append(png)
            pngs += [_damage(rng, png)[1] for _ in range(6)]
    for desired in (4, 3):
        n_ok, n_bad = _check(enc, pngs, desired)
        assert n_ok >= 12 and n_bad >= 12
    _check(enc, pngs, 4, device=True)
    # 8K frames: stripes (1-pass and 2-pass) against a gradient, device-resident
    w, h = 7680, 4320
    pal = np.random.default_rng(3).integers(0, 256, (5, 4), dtype=np.uint8)
    stripes = np.ascontiguousarray((pal[np.arange(w) % 5][None] + (np.arange(h)[:, None, None] * 7).astype(np.uint8)).astype(np.uint8))
    import fpng_amd
    frames = [torch.from_numpy(stripes).cuda(), torch.from_numpy(fpng_amd.synth_image("blocks", w, h, 4)).cuda(), torch.from_numpy(fpng_amd.synth_image("grad", w, h, 4)).cuda()]
    times = {}
    for flags in (0, 1):
        files, _ = enc.encode_tensors(frames, flags)
        for k, (f, t) in enumerate(zip(files, frames)):
            dev = _device_files([f])
            for rep in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                (st, px, cf), = enc.decode_device(dev, 4, [(w, h)])
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                times[(flags, k)] = min(times.get((flags, k), 1e9), dt)
            assert st == 0 and torch.equal(px, t), (flags, k)
    print("periodic 8K decode times (ms):", {k: round(v * 1e3, 2) for k, v in times.items()})
    for flags in (0, 1):
        assert times[(flags, 0)] < 3 * times[(flags, 2)] + 2e-3 and times[(flags, 1)] < 3 * times[(flags, 2)] + 2e-3, times


def test_dropin_decode_memory_uses_the_gpu_for_large_images(enc):
    """fpng::fpng_decode_memory (libfpng.so): images of 256K pixels and more go through fpng_amd_decode_host.  Pixels and status
    codes must be the REFERENCE decoder's (oracle/_ref): the photograph, synthetic frames of all three encode modes incl. a stored
    one, 3 and 4 channels out, and damaged copies of a 1 MP file (bit flips, truncations; a file the GPU path leaves undecided
    falls through to the CPU decoder).  Small images stay on the CPU decoder."""
    import torch
    import fpng_amd
    from cpu_ref import have_ref, ref
    if not have_ref():
        pytest.skip("reference build not available")
    imgs = real_image.variants(real_image.rgb_pixels(dropin.decode))
    ts = [torch.from_numpy(imgs["rgb"]).cuda(), torch.from_numpy(imgs["rgba_ga"]).cuda(), torch.from_numpy(fpng_amd.synth_image("grad", 3840, 2160, 4)).cuda(),
          torch.from_numpy(fpng_amd.synth_image("noise", 1920, 1080, 3)).cuda(), torch.from_numpy(fpng_amd.synth_image("blocks", 1024, 1024, 4)).cuda()]
    n0 = dropin.gpu_decodes()
    calls = 0
    for flags in (0, 1):
        pngs, _ = enc.encode_tensors(ts, flags)
        for png in pngs:
            for desired in (3, 4):
                st_r, out_r, w_r, h_r, c_r = ref().decode(png, desired)
                st, out, w, h, c = dropin.decode(png, desired)
                calls += 1
                assert (st, w, h, c) == (st_r, w_r, h_r, c_r) and st == 0
                assert np.array_equal(out, out_r)
    assert dropin.gpu_decodes() - n0 == calls  # every one of them was answered by the GPU tier
    # damaged copies of a 1 MP file
    rng = np.random.default_rng(21)
    (base,), _ = enc.encode_tensors([torch.from_numpy(fpng_amd.synth_image("grad", 1024, 1024, 3)).cuda()], 0)
    bad = [base[:n] for n in (40, 57, 1000, len(base) // 2, len(base) - 20, len(base) - 1)]
    for _ in range(40):
        d = bytearray(base)
        for _ in range(int(rng.integers(1, 4))):
            d[int(rng.integers(0, len(d)))] ^= 1 << int(rng.integers(0, 8))
        bad.append(bytes(d))
    n_ok = n_bad = 0
    for png in bad:
        st_r, out_r, *_ = ref().decode(png, 4)
        st, out, *_ = dropin.decode(png, 4)
        assert st == st_r
        if st == 0:
            assert np.array_equal(out, out_r)
            n_ok += 1
        else:
            n_bad += 1
    assert n_ok >= 1 and n_bad >= 20
    # a small image: the CPU decoder's
    n1 = dropin.gpu_decodes()
    small = oracle().encode(fpng_amd.synth_image("grad", 300, 200, 4), 300, 200, 4, 0)
    st, out, w, h, c = dropin.decode(small, 4)
    assert st == 0 and dropin.gpu_decodes() == n1


def test_decode_host_one_file_host_to_host(enc):
    """fpng_amd_decode_host through the Python mirror: pixels equal the input, damaged container -> the reference's status code,
    nothing reserved for a file that does not decode."""
    import torch
    import fpng_amd
    for (kind, w, h, c) in (("grad", 1920, 1080, 4), ("blocks", 700, 500, 3), ("noise", 300, 200, 3)):
        img = fpng_amd.synth_image(kind, w, h, c)
        (png,), _ = enc.encode_tensors([torch.from_numpy(img).cuda()], 0)
        for desired in (3, 4):
            st, px, cf = enc.decode_host(png, desired)
            assert st == 0 and cf == c and px.shape == (h, w, desired)
            want = img[:, :, :desired] if c >= desired else np.concatenate([img, np.full((h, w, 1), 255, dtype=np.uint8)], axis=2)
            assert np.array_equal(px, want)
        bad = bytearray(png)
        bad[20] ^= 0x40  # IHDR payload: header CRC mismatch
        st, px, cf = enc.decode_host(bytes(bad), 4)
        cst, *_ = dropin.decode(bytes(bad), 4)
        assert st == cst != 0 and px is None


def test_8k_frame_round_trip(enc):
    import torch
    import fpng_amd
    t = torch.from_numpy(fpng_amd.synth_image("grad", 7680, 4320, 4)).cuda()
    (png,), _ = enc.encode_tensors([t], 0)
    ((st, px, cf),) = enc.decode_batch([png], 4)
    assert st == 0 and cf == 4 and torch.equal(px, t)


def _damaged(rng, base, n_flips, cuts):
    out = [base[:n] for n in cuts]
    for _ in range(n_flips):
        d = bytearray(base)
        for _ in range(int(rng.integers(1, 4))):
            d[int(rng.integers(0, len(d)))] ^= 1 << int(rng.integers(0, 8))
        out.append(bytes(d))
    return out


def test_damaged_files_get_the_reference_status(enc):
    """Truncations, bit flips in the container and in the pixel stream, a wrong block type: the status is the reference decoder's,
    pixels equal wherever both succeed (a flipped bit inside a literal still decodes); host- and device-resident files."""
    import fpng_amd
    rng = np.random.default_rng(12)
    base = [oracle().encode(fpng_amd.synth_image("grad", 300, 200, 4), 300, 200, 4, 0),
            oracle().encode(fpng_amd.synth_image("blocks", 257, 190, 3), 257, 190, 3, 1),
            oracle().encode(fpng_amd.synth_image("noise", 64, 64, 3), 64, 64, 3, 0)]
    pngs = []
    for b in base:
        pngs += _damaged(rng, b, 40, (7, 30, 57, 70, len(b) // 2, len(b) - 17, len(b) - 1))
        d = bytearray(b)
        d[60] ^= 0x06  # block type bits
        pngs.append(bytes(d))
    for device in (False, True):
        n_ok, n_bad = _check(enc, pngs, 4, device=device)
        assert n_ok > 3 and n_bad > 60


def test_damaged_large_files(enc):
    """Damage in files that span many workgroups and several upload groups: an 8K frame (58 MB) and the tiled photograph (11 MP),
    truncated at many places, bits flipped all over the stream (a flipped bit can create a false end-of-block symbol 30 MB in, a
    length symbol that runs over a row end, an invalid code), block type / code length header edits.  The reference's decoder is the
    judge for status AND pixels; batches go through both entry points."""
    import torch
    import fpng_amd
    if not have_ref():
        pytest.skip("reference build not available")
    rng = np.random.default_rng(77)
    imgs = real_image.variants(real_image.rgb_pixels(judge))
    sources = [(torch.from_numpy(fpng_amd.synth_image("grad", 7680, 4320, 4)).cuda(), 0, 120), (torch.from_numpy(imgs["rgb_t4"]).cuda(), 1, 160)]
    for t, flags, n in sources:
        (base,), _ = enc.encode_tensors([t], flags)
        L = len(base)
        bad = []
        for k in range(n):
            d = bytearray(base)
            kind = k % 4
            if kind == 0:    # one flipped bit, stratified over the stream
                i = 60 + (L - 80) * k // n + int(rng.integers(0, 1000))
                d[min(i, L - 1)] ^= 1 << int(rng.integers(0, 8))
            elif kind == 1:  # truncation (the IDAT length no longer fits: chunk parsing), stratified
                d = d[: 58 + (L - 58) * (k + 1) // (n + 1)]
            elif kind == 2:  # a damaged byte in the dynamic block header
                d[int(rng.integers(60, 120))] = int(rng.integers(0, 256))
            else:            # a burst of 4 damaged bytes somewhere
                i = int(rng.integers(200, L - 30))
                d[i:i + 4] = bytes(int(v) for v in rng.integers(0, 256, 4))
            bad.append(bytes(d))
        for device in (False, True):
            half = bad[: len(bad) // 2] if device else bad[len(bad) // 2:]
            for j in range(0, len(half), 4):
                n_ok, n_bad = _check(enc, half[j:j + 4], 4 if t.shape[2] == 4 else 3, device=device)


def test_forced_undecided_falls_through_to_the_cpu_decoder(enc):
    """FPNG_AMD_DECODE_MAX_ROUNDS=0 makes the GPU path leave every compressed file undecided: fpng_amd_decode_batch says so, and
    fpng::fpng_decode_memory (the drop-in) answers with the CPU decoder's pixels all the same."""
    import torch
    import fpng_amd
    t = torch.from_numpy(fpng_amd.synth_image("grad", 1024, 768, 4)).cuda()
    (png,), _ = enc.encode_tensors([t], 0)
    os.environ["FPNG_AMD_DECODE_MAX_ROUNDS"] = "0"
    try:
        ((st, px, cf),) = enc.decode_batch([png], 4)
        assert st == UNDECIDED and px is None
        n0 = dropin.gpu_decodes()
        st, out, w, h, c = dropin.decode(png, 4)
        assert st == 0 and np.array_equal(out, t.cpu().numpy().reshape(-1))
    finally:
        del os.environ["FPNG_AMD_DECODE_MAX_ROUNDS"]
    ((st, px, cf),) = enc.decode_batch([png], 4)
    assert st == 0 and torch.equal(px, t)


def test_device_resident_files(enc):
    """fpng_amd_decode_batch_device: the encoder's own outputs, still in device memory, decoded in place (only a head and a tail of
    each file visit the host): 1-pass, 2-pass and stored files, a file smaller than the head, every address alignment."""
    import torch
    import fpng_amd
    ts = [torch.from_numpy(fpng_amd.synth_image("grad", 3840, 2160, 4, seed=7)).cuda(), torch.from_numpy(fpng_amd.synth_image("noise", 640, 480, 3)).cuda(),
          torch.from_numpy(fpng_amd.synth_image("solid", 16, 4, 4)).cuda(), torch.from_numpy(fpng_amd.synth_image("blocks", 1920, 1080, 3)).cuda(),
          torch.from_numpy(fpng_amd.synth_image("grad", 1000, 1000, 3, seed=9)).cuda()]
    for flags in (0, 1, 2):
        pngs, _ = enc.encode_tensors(ts, flags)
        for shift in (0, 1, 2, 3):
            for desired in (4, 3):
                got = enc.decode_device(_device_files(pngs, shift=shift), desired, [(t.shape[1], t.shape[0]) for t in ts])
                for t, (st, px, cf) in zip(ts, got):
                    assert st == 0 and cf == t.shape[2]
                    want = t[:, :, :desired] if t.shape[2] >= desired else torch.cat([t, torch.full_like(t[:, :, :1], 255)], dim=2)
                    assert torch.equal(px, want)


def test_decode_memory_from_many_threads_at_once(enc):
    """fpng::fpng_decode_memory is re-entrant in the reference; here six threads decode six different files of 1 MP and
    more at once through the GPU tier, three times each, plus a damaged one: every thread gets the reference decoder's status and
    pixels every time."""
    import torch
    import fpng_amd
    frames = [fpng_amd.synth_image("grad", 1280, 1024, 4, seed=3), fpng_amd.synth_image("grad", 1920, 1080, 3, seed=4), fpng_amd.synth_image("blocks", 2048, 1024, 4),
              fpng_amd.synth_image("noise", 1024, 1024, 3), fpng_amd.synth_image("grad", 3840, 2160, 4, seed=5), fpng_amd.synth_image("solid", 1500, 900, 4)]
    pngs, _ = enc.encode_tensors([torch.from_numpy(f).cuda() for f in frames], 0)
    bad = bytearray(pngs[0])
    bad[len(bad) // 2] ^= 0x10
    pngs = list(pngs) + [bytes(bad)]
    n0 = dropin.gpu_decodes()
    for desired in (4, 3):
        got, agree = dropin.decode_threads(pngs, desired, reps=3)
        assert agree
        for png, (st, px) in zip(pngs, got):
            st_r, px_r, *_ = judge(png, desired)
            assert st == st_r
            if st == 0:
                assert np.array_equal(px, px_r)
    assert dropin.gpu_decodes() - n0 >= 2 * 3 * 6


def test_decode_file_goes_through_the_gpu_tier(enc, tmp_path):
    """fpng::fpng_decode_file (reference src/fpng.cpp:3141-3222) of a large file: read, then the same path as fpng_decode_memory."""
    import torch
    import fpng_amd
    img = fpng_amd.synth_image("grad", 2000, 1500, 3)
    (png,), _ = enc.encode_tensors([torch.from_numpy(img).cuda()], 1)
    path = str(tmp_path / "big.png")
    with open(path, "wb") as f:
        f.write(png)
    n0 = dropin.gpu_decodes()
    for desired in (3, 4):
        st, px, w, h, c = dropin.decode_file(path, desired)
        assert st == 0 and (w, h, c) == (2000, 1500, 3)
        st_r, px_r, *_ = judge(png, desired)
        assert np.array_equal(px, px_r)
    assert dropin.gpu_decodes() - n0 == 2


def test_command_line_decoder_fuzz_mode(enc, tmp_path):
    """fpng_amd_test -f (the reference harness's decoder fuzz mode, fpng_test.cpp:1092-1114, which its README drives with zzuf) on
    damaged copies of a 1.9 MP file, the reference's decoder looking at the same bytes (--judge: exit code 2 on any difference in
    status or pixels): the tool either writes out.png or reports the failure, as the reference's does."""
    import subprocess
    import torch
    import fpng_amd
    if not have_ref():
        pytest.skip("reference build not available")
    exe = os.path.join(ROOT, "fpng_amd", "lib", "fpng_amd_test")
    lib = os.path.join(ROOT, "oracle", "_ref", "libfpng_ref.so")
    env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD"}
    (base,), _ = enc.encode_tensors([torch.from_numpy(fpng_amd.synth_image("grad", 1600, 1200, 3)).cuda()], 0)
    rng = np.random.default_rng(5)
    files = [base] + _damaged(rng, base, 24, (100, len(base) // 3, len(base) - 5))
    n_ok = n_fail = 0
    for k, data in enumerate(files):
        path = str(tmp_path / f"f{k}.png")
        with open(path, "wb") as f:
            f.write(data)
        r = subprocess.run([exe, "--judge", lib, "-f", path], capture_output=True, text=True, timeout=300, env=env, cwd=str(tmp_path))
        assert r.returncode in (0, 1), (k, r.returncode, r.stdout[-300:], r.stderr[-300:])
        if r.returncode == 0:
            assert "Wrote out.png 1600x1200 3" in r.stdout
            n_ok += 1
        else:
            assert "fpng::fpng_decode() failed with error" in r.stderr
            n_fail += 1
    assert n_ok >= 1 and n_fail >= 10


def test_a_match_at_a_rows_first_pixel_is_left_to_the_cpu_decoder(enc):
    """tests/golden/first_pixel_match.png (found by tools/emul_campaign.py; tests/test_decode_model.py holds the kernels' logic against
    it on the CPU): one flipped bit makes the first token of a row a match.  The reference decodes the file; both batch entry
    points must leave it to the CPU decoder (never NOT_FPNG), next to valid files that decode, and the drop-in gives the reference's pixels."""
    import torch
    import fpng_amd
    bad = open(os.path.join(ROOT, "tests", "golden", "first_pixel_match.png"), "rb").read()
    t = torch.from_numpy(fpng_amd.synth_image("grad", 300, 40, 4)).cuda()
    (good,), _ = enc.encode_tensors([t], 1)
    for desired in (3, 4):
        cst, cpx, w, h, c = judge(bad, desired)
        assert cst == 0 and (w, h, c) == (65, 16, 4)
        for got in (enc.decode_batch([good, bad, good], desired), enc.decode_device(_device_files([good, bad, good], shift=1), desired, [(300, 40), (65, 16), (300, 40)])):
            assert [st for st, _, _ in got] == [0, UNDECIDED, 0]
            assert torch.equal(got[0][1], t[:, :, :desired]) and torch.equal(got[2][1], t[:, :, :desired])
        dst, dpx, *_ = dropin.decode(bad, desired)
        assert dst == 0 and np.array_equal(np.asarray(dpx)[: w * h * desired], np.asarray(cpx)[: w * h * desired])


@pytest.mark.parametrize("device", [False, True])
def test_edited_token_streams_get_the_references_answer(enc, device):
    """tests/token_mutator.py through the kernels: valid code streams whose tokens bend or break the decoder's semantic rules (matches
    lengthened, split, off a pixel boundary, at a row's first pixel, over the row's end, filter literals changed, the end-of-block
    symbol moved ...).  Status and pixels of the reference's decoder; the kernels may say UNDECIDED only where their logic does (the
    emulator at their constants: a match at a row's first pixel ...), and the drop-in's CPU decoder must then give them."""
    from test_decode_model import CONFIGS, edited_files, emul_decode
    rng = np.random.default_rng(77)
    files = edited_files(rng, 60)
    pngs = [f for _, f in files]
    for desired in (3, 4):
        if device:
            import struct
            dims = [struct.unpack(">II", bytes(p[16:24])) for p in pngs]
            got = enc.decode_device(_device_files(pngs, shift=1), desired, dims)
        else:
            got = enc.decode_batch(pngs, desired)
        accepted = left = 0
        for (name, png), (st, px, cf) in zip(files, got):
            cst, cpx, w, h, c = judge(png, desired)
            if st == UNDECIDED:
                assert emul_decode(png, desired, CONFIGS[0], border_rounds=63)[0] == UNDECIDED, name  # (63: the GPU's border rounds)
                left += 1
                os.environ["FPNG_AMD_DECODE_CPU"] = "1"
                try:
                    dst, dpx, *_ = dropin.decode(png, desired)
                finally:
                    del os.environ["FPNG_AMD_DECODE_CPU"]
                assert dst == cst and (cst != 0 or np.array_equal(np.asarray(dpx)[: w * h * desired], np.asarray(cpx)[: w * h * desired])), name
                continue
            assert st == cst, (name, st, cst)
            if st == 0:
                accepted += 1
                assert np.array_equal(px.cpu().numpy().reshape(-1), np.asarray(cpx)[: w * h * desired]), name
        assert accepted >= 150 and left >= 10, (accepted, left)


@pytest.mark.parametrize("device", [False, True])
def test_container_and_block_edits_get_the_references_answer(enc, device):
    """tests/container_mutator.py through both batch entry points (host files: the whole container is parsed; device-resident files:
    only a head and a tail visit the host, anything unusual makes the whole file come back): chunks inserted / missing / doubled /
    out of order, IHDR fields and dimensions changed, several IDATs, junk behind IEND, other zlib headers and block types, stored
    blocks of other sizes or with damaged headers, the one zero byte behind a stored image that the reference lets pass, dynamic
    headers with other counts -- all with good CRCs.  Status, geometry and pixels of the reference; UNDECIDED only where the
    drop-in's CPU decoder then gives the reference's answer."""
    import container_mutator as CM
    from test_dropin_decode import edited_containers
    rng = np.random.default_rng(88)
    files = edited_containers(rng, 50)
    for (w, h, c) in ((5, 4, 4), (300, 250, 3)):
        img = rng.integers(0, 256, w * h * c, dtype=np.uint8)
        png = oracle().encode(img, w, h, c, 2)
        files += [("stored_tail", CM.stored_with_tail(png, tail)) for tail in (b"", b"\0", b"\1", b"\0\0")]
    pngs = [f for _, f in files]
    for desired in (3, 4):
        judged = [judge(p, desired) for p in pngs]
        if device:
            dims = [(w, h) if st == 0 or w else (0, 0) for st, _, w, h, _ in judged]
            got = enc.decode_device(_device_files(pngs, shift=1), desired, dims)
        else:
            got = enc.decode_batch(pngs, desired)
        accepted = left = 0
        for (name, png), (cst, cpx, w, h, c), (st, px, cf) in zip(files, judged, got):
            if st == UNDECIDED:
                left += 1
                os.environ["FPNG_AMD_DECODE_CPU"] = "1"
                try:
                    dst, dpx, *_ = dropin.decode(png, desired)
                finally:
                    del os.environ["FPNG_AMD_DECODE_CPU"]
                assert dst == cst and (cst != 0 or np.array_equal(np.asarray(dpx)[: w * h * desired], np.asarray(cpx)[: w * h * desired])), name
                continue
            assert st == cst, (name, st, cst)
            if st == 0:
                accepted += 1
                assert cf == c and np.array_equal(px.cpu().numpy().reshape(-1), np.asarray(cpx)[: w * h * desired]), name
        assert accepted >= 50 and left >= 5, (accepted, left)


@pytest.mark.parametrize("device", [False, True])
def test_other_huffman_tables_and_the_reserved_length_symbols(enc, device):
    """tests/header_mutator.py through the kernels -- dec_build_lut_kernel builds the lookup tables of these files on the GPU: random
    complete codes up to 12 bits, single-code tables, every symbol coded, other HLIT / HDIST / HCLEN, distance tables of every shape,
    codes for the reserved length symbols 286 / 287 (left to the CPU decoder, which follows the reference's 4-channel decoder).
    Status and pixels of the reference."""
    from test_dropin_decode import other_tables
    rng = np.random.default_rng(99)
    files = other_tables(rng, 40)
    pngs = [f for _, _, f in files]
    for desired in (3, 4):
        judged = [judge(p, desired) for p in pngs]
        if device:
            got = enc.decode_device(_device_files(pngs, shift=1), desired, [(w, h) for _, _, w, h, _ in judged])
        else:
            got = enc.decode_batch(pngs, desired)
        accepted = left = 0
        for (name, _, png), (cst, cpx, w, h, c), (st, px, cf) in zip(files, judged, got):
            if st == UNDECIDED:
                left += 1
                os.environ["FPNG_AMD_DECODE_CPU"] = "1"
                try:
                    dst, dpx, *_ = dropin.decode(png, desired)
                finally:
                    del os.environ["FPNG_AMD_DECODE_CPU"]
                assert dst == cst and (cst != 0 or np.array_equal(np.asarray(dpx)[: w * h * desired], np.asarray(cpx)[: w * h * desired])), name
                continue
            assert st == cst, (name, st, cst)
            if st == 0:
                accepted += 1
                assert cf == c and np.array_equal(px.cpu().numpy().reshape(-1), np.asarray(cpx)[: w * h * desired]), name
        assert accepted >= 50 and left >= 10, (accepted, left)


@pytest.mark.skipif(not have_ref(), reason="the reference's decoder is the judge")
@pytest.mark.parametrize("case", ["4k_rgba_streamed", "1080p_rgb_glyphs_2pass", "blocks_rgb"])
def test_token_edited_megapixel_files(enc, case):
    """tests/token_mutator.py on MEGAPIXEL files (LargeStream / mutate_large: one local edit at a random place of a token stream that
    spans hundreds of workgroups -- a match lengthened over a row's end, off a pixel boundary, an end-of-block symbol moved, a
    filter literal changed ...), through fpng_amd_decode_batch, fpng_amd_decode_batch_device and fpng::fpng_decode_memory (which
    STREAMS the 4K file: more than 8 MiB of IDAT; semantics src/fpng.cpp:2587-2901).  Status and pixels of the reference's decoder
    at both channel counts; UNDECIDED only for a match at a row's first pixel (lit2match_firstpx), and the drop-in's CPU decoder
    must then give the reference's answer."""
    import struct
    import fpng_amd
    import test_decode_model as M
    import token_mutator as TM
    import ui_images
    img, w, h, c, flags = {
        "4k_rgba_streamed": lambda: (np.asarray(fpng_amd.synth_image("grad", 3840, 2160, 4)).reshape(-1), 3840, 2160, 4, 0),
        "1080p_rgb_glyphs_2pass": lambda: (np.ascontiguousarray(ui_images.glyphs(1920, 1080, 3, seed=5)).reshape(-1), 1920, 1080, 3, 1),
        "blocks_rgb": lambda: (np.asarray(fpng_amd.synth_image("blocks", 2048, 1500, 3)).reshape(-1), 2048, 1500, 3, 0),
    }[case]()
    rng = np.random.default_rng({"4k_rgba_streamed": 3, "1080p_rgb_glyphs_2pass": 1, "blocks_rgb": 1}[case])  # (seeds whose edits the reference both accepts and rejects)
    base = ref().encode(img, w, h, c, flags)
    if case == "4k_rgba_streamed":
        assert len(base) > (8 << 20) + 100
    s = TM.LargeStream(base, M.plan, M.emul())
    files = [(name, f) for name, f in (TM.mutate_large(s, rng) for _ in range(20)) if f is not None]
    assert len(files) >= 6
    rejected = 0
    for desired in (3, 4):
        judged = [ref().decode(f, desired) for _, f in files]
        dims = [struct.unpack(">II", bytes(f[16:24])) for _, f in files]
        for got in (enc.decode_batch([f for _, f in files], desired), enc.decode_device(_device_files([f for _, f in files], shift=2), desired, dims)):
            for (name, f), (cst, cpx, *_), (st, px, _) in zip(files, judged, got):
                if st == UNDECIDED:
                    assert name == "lit2match_firstpx", (name, st, cst)
                    os.environ["FPNG_AMD_DECODE_CPU"] = "1"
                    try:
                        st, dpx, *_ = dropin.decode(f, desired)
                    finally:
                        del os.environ["FPNG_AMD_DECODE_CPU"]
                    assert st == cst and (cst != 0 or np.array_equal(np.asarray(dpx)[: w * h * desired], np.asarray(cpx)[: w * h * desired])), name
                else:
                    assert st == cst, (name, st, cst)
                    assert cst != 0 or np.array_equal(px.cpu().numpy().reshape(-1), np.asarray(cpx)[: w * h * desired]), name
        before = dropin.shim().shim_gpu_decodes()
        for (name, f), (cst, cpx, *_) in zip(files, judged):  # the drop-in itself (GPU tier; streamed where the IDAT is large)
            st, dpx, *_ = dropin.decode(f, desired)
            assert st == cst and (cst != 0 or np.array_equal(np.asarray(dpx)[: w * h * desired], np.asarray(cpx)[: w * h * desired])), name
            rejected += cst != 0
        assert dropin.shim().shim_gpu_decodes() > before
    assert rejected >= 2  # (one rejected file, at both channel counts)


@pytest.mark.skipif(not have_ref(), reason="the reference's decoder is the judge")
def test_damaged_8k_files_through_the_streamed_host_path(enc):
    """fpng_amd_decode_host / fpng::fpng_decode_memory STREAM a file from 8 MiB of IDAT on: a piece's rows are un-filtered on a
    stream of their own while the next piece is synchronised and decoded, and those kernels may set the file's status bits at any
    moment.  dec_unfilter_kernel must not let such a bit split one launch's workgroups into some that publish their look-back sums
    and some that leave (the others would spin up to the limit: a multi-second stall, found by review in round 4) -- in the streamed
    form no workgroup skips.  Damaged 8K files (flipped bits stratified over 58 MB, bursts, a damaged header): the reference's
    status, its pixels where it succeeds, and no call takes long."""
    import time
    import torch
    import fpng_amd
    rng = np.random.default_rng(4242)
    (base,), _ = enc.encode_tensors([torch.from_numpy(fpng_amd.synth_image("grad", 7680, 4320, 4)).cuda()], 0)
    L = len(base)
    files = []
    for k in range(10):
        d = bytearray(base)
        if k % 3 == 0:
            d[60 + (L - 80) * k // 10 + int(rng.integers(0, 1000))] ^= 1 << int(rng.integers(0, 8))
        elif k % 3 == 1:
            i = int(rng.integers(200, L - 30))
            d[i:i + 4] = bytes(int(v) for v in rng.integers(0, 256, 4))
        else:
            for _ in range(3):
                d[int(rng.integers(L // 2, L - 30))] ^= 0xFF
        files.append(bytes(d))
    dropin.decode(base, 4)  # (warm: buffers, streams)
    n_bad = 0
    slowest = 0.0
    for f in files:
        cst, cpx, w, h, c = ref().decode(f, 4)
        t0 = time.perf_counter()
        st, px, *_ = dropin.decode(f, 4)
        slowest = max(slowest, time.perf_counter() - t0)
        assert st == cst
        if cst == 0:
            assert np.array_equal(np.asarray(px), np.asarray(cpx)[: w * h * 4])
        n_bad += cst != 0
    assert n_bad >= 5
    # (dropin.decode() allocates and copies ~270 MB around the call: ~0.15 s; a stalled look-back costs seconds)
    assert slowest < 1.0, slowest
