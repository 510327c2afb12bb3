"""Images past 2 GiB, end to end (-m gpu): the top three quarters of the size range the encoder accepts (check_dims: up to 0xFFFFFF00
filtered bytes) and the decoder returns (up to 2^30 pixels).  Encodes are judged by the UNMODIFIED reference's files
(tests/golden/large.json, oracle/make_golden_large.py), decodes by the source image, compared on the device in row chunks.

What only breaks here: input and output byte offsets past 2^31, token bit positions past 2^32 (zlib streams over 512 MiB), stored
block indices past 32768, CRC-32 / Adler-32 over such files, decoder output offsets past 2^31 -- and the stored outcome whose
58 + zlib size passes UINT32_MAX, which the reference refuses (its buffer size is a uint32_t sum, src/fpng.cpp:1747) and so must we.

Every test asserts the property it exists for, so that a change of shape cannot quietly make it small again.
"""
import hashlib
import json
import os

import numpy as np
import pytest

from cpu_ref import ROOT

pytestmark = pytest.mark.gpu

FORCE_UNCOMPRESSED = 2
STATUS_STORED_TOO_LARGE = 1  # FPNG_AMD_STATUS_STORED_TOO_LARGE (include/fpng_amd.h)
ERR_UNSUPPORTED = -6         # FPNG_AMD_ERR_UNSUPPORTED
ROWS = 2048                  # rows per comparison chunk


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(ROOT, "tests", "golden", "large.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def enc(built_lib):
    import torch
    import fpng_amd
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    e = fpng_amd.Encoder(device=0)
    yield e
    e.close()
    fpng_amd.release_cached_memory()


@pytest.fixture(scope="module")
def files():
    """fpng files of the flags-0 encodes, kept on the device for the decode tests: name -> (uint8 CUDA tensor of the file's bytes)"""
    return {}


_peak = [0]


@pytest.fixture(autouse=True)
def _device_memory(enc):
    """device memory in use after each test (the library's cached scratch included); the module's peak is printed at the end"""
    import torch
    yield
    free, total = torch.cuda.mem_get_info(0)
    _peak[0] = max(_peak[0], total - free)


@pytest.fixture(scope="module", autouse=True)
def _report_peak():
    import torch
    free, total = torch.cuda.mem_get_info(0)
    yield
    print(f"\ntest_gpu_large: device memory in use (whole card): {(total - free) / 2**30:.1f} GiB before the module, "
          f"{_peak[0] / 2**30:.1f} GiB at the peak after a test")


def _host(gold, name):
    import fpng_amd
    g = gold[name]
    return fpng_amd.synth_image(g["kind"], g["w"], g["h"], g["c"], seed=gold["seed"])


def _device(gold, name):
    import torch
    return torch.from_numpy(_host(gold, name)).cuda()


def _n_filtered(g):
    return (g["w"] * g["c"] + 1) * g["h"]


def _sha(t):
    """sha256 of a uint8 CUDA tensor, downloaded 256 MiB at a time"""
    h = hashlib.sha256()
    for i in range(0, t.numel(), 1 << 28):
        h.update(t[i:i + (1 << 28)].cpu().numpy().tobytes())
    return h.hexdigest()


def _submit(enc, img, flags, ex=None):
    """one image through submit (ex = (order, bottom_up): submit_ex) -> (output tensor, png_size, mode, status)"""
    import torch
    import fpng_amd
    h, w, c = img.shape
    out = torch.empty(fpng_amd.max_encoded_size(w, h, c) + 64, dtype=torch.uint8, device="cuda")
    out[:64].fill_(0xAB)
    if ex is None:
        enc.submit([img], [out], flags)
    else:
        enc.submit_ex([img], [out], flags, order=ex[0], bottom_up=ex[1])
    (size, mode, status), = enc.wait(enc.last_ticket, 1)
    return out, size, mode, status


def _check_file(out, size, mode, status, exp, what):
    assert status == 0, f"{what}: status {status}"
    assert size == exp["size"], f"{what}: {size} bytes, reference {exp['size']}"
    assert int.from_bytes(out[50:54].cpu().numpy().tobytes(), "big") == exp["idat_len"], f"{what}: IDAT length"
    assert _sha(out[:size]) == exp["sha256"], f"{what}: the file differs from the reference's"


def _check_refused(out, size, status, what):
    assert status == STATUS_STORED_TOO_LARGE and size == 0, f"{what}: (size {size}, status {status}), the reference returns false"
    assert bool((out[:64] == 0xAB).all()), f"{what}: a refused file must not be written"


def _encode_case(enc, gold, files, name, flags_list):
    import torch
    g = gold[name]
    img = _device(gold, name)
    assert img.numel() > 2**31 and _n_filtered(g) > 2**31  # input bytes past 2^31
    done = {}
    for fl in flags_list:
        exp = g["flags"][str(fl)]
        out, size, mode, status = _submit(enc, img, fl)
        what = f"{name} flags {fl}"
        if exp is None:
            _check_refused(out, size, status, what)
        else:
            _check_file(out, size, mode, status, exp, what)
            done[fl] = (size, mode)
            if fl == 0 and name in ("G1", "G3", "G4"):
                files[name] = out[:size]
        del out
        torch.cuda.empty_cache()
    return done


# ---------------------------------------------------------------------------------------------------------------------------
# encode


def test_g1_rgba_24000_squared_1pass_2pass_and_forced_stored(enc, gold, files):
    """2.3 GB of RGBA: a 1-pass IDAT of about 1 GB (token bits past 2^32), the 2-pass histogram and table builder, and forced stored
    blocks past 2^31 bytes"""
    g = gold["G1"]
    assert g["flags"]["0"]["idat_len"] > 2**29 and g["flags"]["1"]["idat_len"] > 2**29
    assert g["flags"]["2"]["size"] > 2**31
    done = _encode_case(enc, gold, files, "G1", [0, 1, 2])
    assert done[0][1] == 0 and done[1][1] == 0 and done[2][1] == 1


def test_g3_rgb_walk_past_2gib(enc, gold, files):
    """encode_rows<3> over 2.16 GB of RGB"""
    assert gold["G3"]["c"] == 3 and gold["G3"]["flags"]["0"]["idat_len"] > 2**29
    done = _encode_case(enc, gold, files, "G3", [0])
    assert done[0][1] == 0


def test_g4_stored_fallback_past_32768_blocks(enc, gold, files):
    """noise: the compressed attempt fails and the stored fallback writes a 3.1 GB file of more than 32768 blocks"""
    g = gold["G4"]
    assert (_n_filtered(g) + 65534) // 65535 > 32768 and g["flags"]["0"]["size"] > 2**31
    done = _encode_case(enc, gold, files, "G4", [0])
    assert done[0][1] == 1


def test_b1_largest_stored_file_the_reference_writes(enc, gold, files):
    """58 + zlib size just under 2^32: written, as the reference does (fallback and forced)"""
    g = gold["B1"]
    for fl in ("0", "2"):
        assert g["flags"][fl] is not None and 58 + g["flags"][fl]["idat_len"] > 2**32 - 2**20
    done = _encode_case(enc, gold, files, "B1", [0, 2])
    assert done[0][1] == 1 and done[2][1] == 1


def test_b2_stored_past_4gib_is_refused(enc, gold, files):
    """two RGBA columns more than B1: the stored file's 58 + zlib size passes UINT32_MAX, the reference returns false (flags 0 and
    FPNG_FORCE_UNCOMPRESSED); the device reports FPNG_AMD_STATUS_STORED_TOO_LARGE and writes nothing"""
    g = gold["B2"]
    n = _n_filtered(g)
    assert 58 + 6 + n + 5 * ((n + 65534) // 65535) > 2**32 - 1
    assert g["flags"]["0"] is None and g["flags"]["2"] is None
    _encode_case(enc, gold, files, "B2", [0, 2])


def test_b3_compressible_at_b2_shape_is_written(enc, gold, files):
    """B2's shape with a gradient: the compressed outcome fits, so the refusal is for stored outcomes only"""
    assert gold["B3"]["w"] == gold["B2"]["w"] and gold["B3"]["h"] == gold["B2"]["h"]
    assert gold["B3"]["flags"]["0"] is not None
    done = _encode_case(enc, gold, files, "B3", [0])
    assert done[0][1] == 0


def test_submit_ex_bottom_up_bgra_gives_g1(enc, gold):
    """G1 handed over as a bottom-up BGRA buffer (2.3 GB, negative pitch) through submit_ex: G1's bytes"""
    import torch
    img = _device(gold, "G1")
    bgra = img[..., [2, 1, 0, 3]].flip(0).contiguous()
    del img
    torch.cuda.empty_cache()
    assert bgra.numel() > 2**31
    out, size, mode, status = _submit(enc, bgra, 0, ex=("bgra", True))
    _check_file(out, size, mode, status, gold["G1"]["flags"]["0"], "G1 as bottom-up BGRA")


def test_encode_host_streamed_g1(enc, gold):
    """fpng_amd_encode_host on G1 in host memory: the streamed row-band pipeline (upload, encode, download overlapped)"""
    img = _host(gold, "G1")
    g = gold["G1"]
    png = enc.encode_host(img, g["w"], g["h"], g["c"], 0)
    assert enc.last_host_bands() > 1, "G1 should be streamed in row bands"
    exp = g["flags"]["0"]
    assert len(png) == exp["size"] and hashlib.sha256(png).hexdigest() == exp["sha256"]


def test_host_paths_refuse_b2(enc, gold):
    """encode_host (the streamed path sends a stored outcome through the whole-image path) and fpng::fpng_encode_image_to_memory on
    B2: refused, with FPNG_AMD_ERR_UNSUPPORTED / false, as the reference returns false"""
    import fpng_amd
    import dropin
    g = gold["B2"]
    img = _host(gold, "B2")
    for fl in (0, FORCE_UNCOMPRESSED):
        with pytest.raises(fpng_amd.FpngAmdError) as ei:
            enc.encode_host(img, g["w"], g["h"], g["c"], fl)
        assert ei.value.code == ERR_UNSUPPORTED, f"encode_host flags {fl}: {ei.value}"
    assert dropin.encode(img, g["w"], g["h"], g["c"], 0) is None


# ---------------------------------------------------------------------------------------------------------------------------
# decode (the files of the encode tests above, which must have passed)


def _file(files, name):
    if name not in files:
        pytest.fail(f"{name}'s file is missing: its encode test failed or did not run")
    return files[name]


def _same_pixels(dec, src, desired, what):
    """decoded (h, w, desired) CUDA tensor or numpy array against the source (h, w, c) CUDA tensor, ROWS rows at a time"""
    import torch
    h, w, c = src.shape
    assert tuple(dec.shape) == (h, w, desired), f"{what}: shape {tuple(dec.shape)}"
    k = min(c, desired)
    for r in range(0, h, ROWS):
        a = dec[r:r + ROWS]
        if not isinstance(a, torch.Tensor):
            a = torch.from_numpy(np.ascontiguousarray(a)).cuda()
        b = src[r:r + ROWS]
        assert torch.equal(a[..., :k], b[..., :k]), f"{what}: rows {r}..{r + ROWS} differ"
        if desired > c:
            assert bool((a[..., 3] == 255).all()), f"{what}: alpha of rows {r}..{r + ROWS}"


def _decode_device(enc, gold, files, name, desired_list):
    import torch
    g = gold[name]
    png = _file(files, name)
    src = _device(gold, name)
    biggest = 0
    for d in desired_list:
        (status, dec, chans), = enc.decode_device([png], d, [(g["w"], g["h"])])
        assert status == 0 and chans == g["c"], f"{name} desired {d}: status {status}"
        biggest = max(biggest, dec.numel())
        _same_pixels(dec, src, d, f"{name} desired {d}")
        del dec
        torch.cuda.empty_cache()
    assert biggest > 2**31  # decoder output offsets past 2^31


def test_decode_device_g1(enc, gold, files):
    _decode_device(enc, gold, files, "G1", [4, 3])


def test_decode_device_g4_stored(enc, gold, files):
    _decode_device(enc, gold, files, "G4", [4, 3])


def test_decode_device_g3(enc, gold, files):
    _decode_device(enc, gold, files, "G3", [3, 4])


def test_decode_host_streamed_g1_g4(enc, gold, files):
    """fpng_amd_decode_host: the file from host memory, streamed upload / decode / download into host memory"""
    import torch
    for name in ("G1", "G4"):
        g = gold[name]
        png = _file(files, name).cpu().numpy()
        status, dec, chans = enc.decode_host(png, 4)
        del png
        assert status == 0 and chans == g["c"], f"{name}: status {status}"
        assert dec.nbytes > 2**31
        src = _device(gold, name)
        _same_pixels(dec, src, 4, f"{name} decode_host")
        del dec, src
        torch.cuda.empty_cache()


def test_dropin_decode_memory_g1(enc, gold, files):
    """fpng::fpng_decode_memory (the C++ drop-in's GPU tier) on G1's 1 GB file"""
    import dropin
    g = gold["G1"]
    png = _file(files, "G1").cpu().numpy()
    status, dec, w, h, c = dropin.decode(png, 4)
    del png
    assert status == 0 and (w, h, c) == (g["w"], g["h"], g["c"]), f"status {status}"
    assert dec.nbytes > 2**31
    _same_pixels(dec.reshape(h, w, 4), _device(gold, "G1"), 4, "G1 fpng_decode_memory")


def test_decode_batch_g1_then_small_files(enc, gold, files):
    """one decode_batch of G1 followed by 8 small files: theirs come after 2.3 GB of G1's pixels and its token records in the group"""
    import torch
    import fpng_amd
    small = [torch.from_numpy(fpng_amd.synth_image(("grad", "blocks")[i % 2], 301 + 37 * i, 97 + 11 * i, 3 + i % 2, seed=50 + i)).cuda()
             for i in range(8)]
    pngs, _ = enc.encode_tensors(small, 0)
    big = _file(files, "G1").cpu().numpy().tobytes()
    res = enc.decode_batch([big] + pngs, 4)
    del big
    assert [r[0] for r in res] == [0] * 9
    assert res[0][1].numel() > 2**31
    _same_pixels(res[0][1], _device(gold, "G1"), 4, "G1 in the batch")
    for i, (im, (status, dec, chans)) in enumerate(zip(small, res[1:])):
        _same_pixels(dec, im, 4, f"small file {i} behind G1")
