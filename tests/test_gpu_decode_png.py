"""The general decode tier on the GPU (-m gpu; fpng_amd_decode_batch(_device)_png, fpng_amd/csrc/png_inflate.hip): ordinary PNG files
against Pillow's pixels, damaged ones against the status table of include/fpng_amd.h and against the host twin of the kernels'
logic (tests/cpp/png_inflate_host.cpp, whose sanitizer build tests/test_png_inflate_cpu.py runs on the same cases).  Every
destination lies between guard bands that must stay untouched."""
import os
import struct
import subprocess

import numpy as np
import pytest

import png_cases as pc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 256


@pytest.fixture(scope="module")
def enc(built_lib):
    import torch
    import fpng_amd
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    e = fpng_amd.Encoder(device=0)
    yield e
    e.close()


def _dims(p):
    if len(p) < 24:
        return 0, 0
    w, h = struct.unpack(">II", bytes(p[16:24]))
    return (w, h) if 0 < w <= 4096 and 0 < h <= 4096 else (0, 0)


def _to_device(files):
    import torch
    blob = torch.frombuffer(bytearray(b"".join(files)), dtype=torch.uint8).cuda() if any(len(f) for f in files) else torch.zeros(1, dtype=torch.uint8, device="cuda")
    out, at = [], 0
    for f in files:
        out.append(blob[at:at + len(f)])
        at += len(f)
    return out


def decode(enc, files, desired, flags=0, host=False, dims=None):
    """-> [(status, pixels as numpy (h, w, desired) or None, channels_in_file)]; asserts that the guard bands are untouched.
    dims: the files' known (w, h), where they are no damaged files whose headers need the cap of _dims"""
    import torch
    sizes = [max(w * h * desired, 1) for w, h in (map(_dims, files) if dims is None else dims)]
    arena = torch.full((sum(sizes) + GUARD * (len(files) + 1),), 0xA5, dtype=torch.uint8, device="cuda")
    outs, at = [], GUARD
    for n in sizes:
        outs.append(arena[at:at + n])
        at += n + GUARD
    if host:
        res = enc.decode_batch_png(list(files), desired, outs=outs, flags=flags)
    else:
        res = enc.decode_device_png(_to_device(files), desired, outs=outs, flags=flags)
    torch.cuda.synchronize()
    a = arena.cpu().numpy()
    at = 0
    for i, n in enumerate(sizes):
        assert (a[at:at + GUARD] == 0xA5).all(), f"guard in front of file {i}"
        at += GUARD + n
    assert (a[at:at + GUARD] == 0xA5).all(), "guard behind the last file"
    return [(st, px.cpu().numpy() if px is not None else None, c) for st, px, c in res]


def check_against_pillow(enc, cases, desired, **kw):
    got = decode(enc, [f for _, f in cases], desired, **kw)
    for (name, f), (st, px, _) in zip(cases, got):
        assert st == 0, (name, st)
        assert np.array_equal(px, pc.expected(f, desired)), name


@pytest.mark.parametrize("desired", [3, 4])
def test_formats(enc, desired):
    """colour types 0, 2, 3, 4, 6; tRNS shorter than PLTE; colour keys on grey and RGB"""
    cases = pc.format_cases()
    check_against_pillow(enc, cases, desired)
    chans = {n: c for (n, _), (_, _, c) in zip(cases, decode(enc, [f for _, f in cases], desired))}
    assert [chans[k] for k in ("color0", "color2", "color3", "color4", "color6", "palette_trns_short")] == [1, 3, 3, 2, 4, 4]


@pytest.mark.parametrize("desired", [3, 4])
def test_shapes_of_the_skewed_band(enc, desired):
    """heights 1, 2, 63, 64, 65, 129 x widths 1, 2, 63, 64, 65, 300; each filter on every row and a random one per row; 1-4 bytes per pixel"""
    check_against_pillow(enc, pc.shape_cases(), desired)


def test_stream_forms(enc):
    """stored blocks (an empty one among them), fixed, Huffman only, RLE, levels 1 / 6 / 9, windows 9 and 15, matches near 32768 that
    cross rows, 15-bit codes, many blocks"""
    cases = pc.stream_cases()
    assert pc.max_code_length(pc.idat_stream(dict(cases)["long_codes"])) == 15
    check_against_pillow(enc, cases, 4)
    check_against_pillow(enc, cases, 3)


def test_hand_built_far_distances(enc):
    """streams no zlib writes: matches of 65 .. 258 bytes at distances 32507 .. 32768, whose stores take the window slots that
    their own later bytes are read from"""
    cases = pc.hand_cases()
    assert {pc.token_stats(pc.idat_stream(f))[1] for _, f in cases} >= set(pc.HAND_DISTANCES)
    assert pc.token_stats(pc.idat_stream(dict(pc.stream_cases())["far_matches"]))[1] == 32436
    check_against_pillow(enc, cases, 4)
    check_against_pillow(enc, cases, 3)


def test_idat_geometry(enc):
    """one chunk, Pillow's own 64 KiB chunks, chunks of 1 / 2 / 3 / 7 bytes, cuts inside the zlib header, a stored LEN and the
    Adler-32, empty IDATs, PLTE behind the fetched head, output beyond the image"""
    check_against_pillow(enc, pc.idat_cases(), 4)
    check_against_pillow(enc, pc.idat_cases(), 3)


def _fpng_files(enc):
    """the project's own encoder: 1-pass and 2-pass, 3 and 4 channels; and the golden file the fast path leaves undecided"""
    import torch
    import fpng_amd
    out = []
    for k, (w, h, c, flags) in enumerate([(97, 61, 3, 0), (97, 61, 4, 0), (130, 40, 3, fpng_amd.FPNG_ENCODE_SLOWER), (130, 40, 4, fpng_amd.FPNG_ENCODE_SLOWER)]):
        img = fpng_amd.synth_image(("grad", "blocks", "noise", "grad")[k], w, h, c)
        (png,), _ = enc.encode_tensors([torch.from_numpy(img).cuda()], flags)
        out.append((f"fpng_{w}x{h}x{c}_{flags}", bytes(png)))
    out.append(("first_pixel_match", open(os.path.join(ROOT, "tests", "golden", "first_pixel_match.png"), "rb").read()))
    return out


@pytest.mark.parametrize("desired", [3, 4])
def test_routing(enc, desired):
    fpng = _fpng_files(enc)
    foreign = pc.format_cases()[:5]
    mixed = [fpng[0], foreign[0], fpng[1], foreign[1], fpng[4], foreign[2], fpng[2], foreign[3], fpng[3], foreign[4]]
    files = [f for _, f in mixed]
    dims = [_dims(f) for f in files]
    fast = enc.decode_device(_to_device(files), desired, dims)
    routed = decode(enc, files, desired)
    general = decode(enc, files, desired, flags=1)
    for (name, f), (st_f, px_f, _), (st_r, px_r, c_r), (st_g, px_g, c_g) in zip(mixed, fast, routed, general):
        assert st_r == 0 and st_g == 0, name
        assert np.array_equal(px_r, px_g) and c_r == c_g, name
        if name == "first_pixel_match":
            # (one flipped bit: the IDAT's CRC and the Adler-32 are off, which Pillow refuses, so it judges the file with both recomputed.  The
            #  match at a row's first pixel copies the bytes in front of it, as inflate has it: the fpng decoders' reading of such
            #  a match -- a pixel of zeros -- is theirs alone, and no fpng encoder writes one)
            assert st_f == pc.UNDECIDED
            f = pc.repair_checksums(f)
        assert np.array_equal(px_r, pc.expected(f, desired)), name
        if name.startswith("fpng_"):
            assert st_f == 0 and np.array_equal(px_r, px_f.cpu().numpy()), name
        elif name != "first_pixel_match":
            assert st_f == pc.NOT_FPNG, name  # (the fpng calls keep their answer for foreign files)


def test_refusals_and_damage(enc):
    cases = pc.damage_cases()
    for host in (False, True):
        got = decode(enc, [f for _, f, _ in cases], 4, host=host)
        for (name, _, want), (st, px, _) in zip(cases, got):
            assert st == want, (name, host)


def test_damaged_files_equal_the_host_twin(enc, tmp_path):
    """a few hundred files of the CPU sweeps (truncations and byte changes): status and pixel hash of the host twin, file by file"""
    exe = str(tmp_path / "png_inflate_host")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "fpng_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "png_inflate_host.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    files = []
    for name, file in pc.sweep_sources():
        sweep = pc.sweep_files(name, file, changes=120)
        files += [file, file[:-12]] + [f for _, f in sweep[40::30]] + [f for _, f in sweep[-120:]]
    paths = []
    for i, f in enumerate(files):
        paths.append(str(tmp_path / f"{i}.png"))
        open(paths[-1], "wb").write(f)
    twin = [ln.split() for ln in subprocess.run([exe, "4"] + paths, capture_output=True, text=True, check=True).stdout.splitlines()]
    got = decode(enc, files, 4)
    assert len(twin) == len(files) >= 300
    statuses = set()
    for i, (t, (st, px, _)) in enumerate(zip(twin, got)):
        assert st == int(t[0]), i
        statuses.add(st)
        if st == 0:
            assert pc.pixel_hash(px.tobytes()) == int(t[4], 16), i
    assert {0, pc.CHUNK_PARSING, pc.INVALID_IDAT} <= statuses


def test_groups_reuse_the_scratch(enc):
    """FPNG_AMD_PNG_SCRATCH_LIMIT so low that the batch needs three groups: the same pixels as in one"""
    cases = [(n, f) for n, f in pc.shape_cases() if "_300x" in n][:6] + pc.format_cases()[:3]
    files = [f for _, f in cases]
    one = decode(enc, files, 4)
    scan = [h * (1 + w * pc.BPP[f[25]]) for f in files for w, h in [_dims(f)]]
    os.environ["FPNG_AMD_PNG_SCRATCH_LIMIT"] = str(sum((s + 255) // 256 * 256 for s in scan) // 3 + 256)
    try:
        three = decode(enc, files, 4)
    finally:
        del os.environ["FPNG_AMD_PNG_SCRATCH_LIMIT"]
    for (name, f), a, b in zip(cases, one, three):
        assert a[0] == 0 and b[0] == 0 and np.array_equal(a[1], b[1]), name
        assert np.array_equal(a[1], pc.expected(f, 4)), name


def test_host_form_equals_device_form(enc):
    mixed = _fpng_files(enc)[:4] + pc.format_cases() + pc.idat_cases()[:3]
    files = [f for _, f in mixed]
    for desired in (3, 4):
        dev, host = decode(enc, files, desired), decode(enc, files, desired, host=True)
        for (name, f), a, b in zip(mixed, dev, host):
            assert a[0] == 0 and b[0] == 0 and a[2] == b[2], name
            assert np.array_equal(a[1], b[1]) and np.array_equal(a[1], pc.expected(f, desired)), name


def test_room_and_argument_rules(enc):
    import torch
    import fpng_amd
    f = pc.format_cases()[1][1]
    dev = _to_device([f])
    small = torch.zeros(16, dtype=torch.uint8, device="cuda")
    with pytest.raises(fpng_amd.FpngAmdError):
        enc.decode_device_png(dev, 4, outs=[small])
    with pytest.raises(fpng_amd.FpngAmdError):
        enc.decode_device_png(dev, 4, flags=2)
    (st, px, c), = enc.decode_device_png(dev, 4)  # (the output sized from the header)
    assert st == 0 and np.array_equal(px.cpu().numpy(), pc.expected(f, 4))
