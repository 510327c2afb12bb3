"""The general decode tier's per-wave logic (fpng_amd/csrc/png_inflate_core.h) on the CPU: tests/cpp/png_inflate_host.cpp runs it lane
by lane, built plainly and with -fsanitize=address,undefined (a stand-alone program, run as a child process).  Expectations are
Pillow's pixels and, for damaged files, the status table of include/fpng_amd.h."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import png_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def twins(tmp_path_factory):
    """(plain build, sanitizer build, a directory for the files)"""
    d = tmp_path_factory.mktemp("png_inflate_host")
    src = os.path.join(ROOT, "tests", "cpp", "png_inflate_host.cpp")
    base = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "fpng_amd", "csrc"), src]
    plain, san = str(d / "png_inflate_host"), str(d / "png_inflate_host_san")
    for exe, extra in ((plain, []), (san, ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DPNGI_GUARD=0"])):
        r = subprocess.run(base + extra + ["-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
    return plain, san, d


def run_twin(exe, d, files, desired, tag):
    """-> [(status, w, h, channels_in_file, hash, guard)] per file; any sanitizer report fails the run (non-zero exit, stderr)"""
    out = []
    for at in range(0, len(files), 400):  # (command lines of a few hundred paths)
        paths = []
        for i, f in enumerate(files[at:at + 400]):
            p = str(d / f"{tag}_{at + i}.png")
            with open(p, "wb") as fh:
                fh.write(f)
            paths.append(p)
        r = subprocess.run([exe, str(desired)] + paths, capture_output=True, text=True)
        for p in paths:
            os.remove(p)
        assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-3000:])
        lines = r.stdout.splitlines()
        assert len(lines) == len(paths)
        out += [(int(a), int(b), int(c), int(e), int(h, 16), int(g)) for a, b, c, e, h, g in (ln.split() for ln in lines)]
    return out


@pytest.mark.parametrize("which", ["plain", "sanitizers"])
@pytest.mark.parametrize("desired", [3, 4])
def test_designed_cases_give_pillows_pixels(twins, which, desired):
    plain, san, d = twins
    cases = pc.designed_cases()
    got = run_twin(plain if which == "plain" else san, d, [f for _, f in cases], desired, f"designed{desired}")
    for (name, f), (status, w, h, chans, hsh, guard) in zip(cases, got):
        exp = pc.expected(f, desired)
        assert status == 0, name
        assert (h, w) == exp.shape[:2], name
        assert hsh == pc.pixel_hash(exp.tobytes()), name
        assert guard == 1, name


def test_channels_in_file(twins):
    plain, _, d = twins
    cases = dict(pc.format_cases())
    names = ["color0", "color2", "color3", "color4", "color6", "palette_trns_short"]
    got = run_twin(plain, d, [cases[k] for k in names], 4, "chans")
    assert [g[3] for g in got] == [1, 3, 3, 2, 4, 4]


def test_far_matches_reach_the_distances_they_are_meant_for():
    """zlib's own streams stop at 32506 (window - MIN_LOOKAHEAD); far_matches gets to 32436 with long matches; the hand-built
    streams, which run with the designed cases above, cover 32507 .. 32768 with lengths above 64"""
    out, far, longest = pc.token_stats(pc.idat_stream(dict(pc.stream_cases())["far_matches"]))
    assert out == 300 * 901 and far == 32436 and longest == 258
    seen = set()
    for name, f in pc.hand_cases():
        out, far, longest = pc.token_stats(pc.idat_stream(f))
        assert out == 98 * 337 and 32507 <= far <= 32768 and longest > 64, name
        seen.add(far)
    assert seen >= set(pc.HAND_DISTANCES)


def test_shape_cases_cross_every_filter_with_every_shape():
    names = {n for n, _ in pc.shape_cases()}
    for h in pc.SHAPE_HEIGHTS:
        for w in pc.SHAPE_WIDTHS:
            for filt in "01234r":
                assert any(n.startswith(f"shape_{w}x{h}_c") and n.endswith(f"_f{filt}") for n in names), (w, h, filt)


def test_long_codes_case_has_15_bit_codes():
    assert pc.max_code_length(pc.idat_stream(dict(pc.stream_cases())["long_codes"])) == 15


@pytest.mark.parametrize("which", ["plain", "sanitizers"])
def test_damage_cases_give_their_status(twins, which):
    plain, san, d = twins
    cases = pc.damage_cases()
    got = run_twin(plain if which == "plain" else san, d, [f for _, f, _ in cases], 4, "damage")
    for (name, f, want), (status, _, _, _, _, guard) in zip(cases, got):
        assert status == want, name
        assert guard == 1, name


@pytest.mark.parametrize("source", [0, 1, 2])
def test_truncation_and_byte_change_sweeps(twins, source):
    """every truncation length and 2000 single-byte changes of a 32 x 32 file: no sanitizer report, nothing written outside the
    image (the sanitizer build has no guard bands: the first byte outside is its), and wherever the status is 0 and Pillow loads
    the file, Pillow's pixels"""
    plain, san, d = twins
    name, file = pc.sweep_sources()[source]
    files = pc.sweep_files(name, file)
    got_san = run_twin(san, d, [f for _, f in files], 4, f"sweep{source}s")
    got = run_twin(plain, d, [f for _, f in files], 4, f"sweep{source}")
    assert got == got_san
    decoded = 0
    for (fname, f), (status, w, h, _, hsh, guard) in zip(files, got):
        assert guard == 1, fname
        if status == 0 and pc.pillow_loads(f):
            exp = pc.expected(f, 4)
            assert (h, w) == exp.shape[:2] and hsh == pc.pixel_hash(exp.tobytes()), fname
            decoded += 1
    assert decoded > 0  # (at least the cuts inside IEND and the changes of the Adler-32, which neither decoder reads, leave both with the pixels)


def test_new_symbols_are_exported_and_declared(built_lib):
    """added after ABI version 5 without changing it: found with dlsym, declared in the header, bound by the package"""
    lib = ctypes.CDLL(built_lib)
    hdr = open(os.path.join(ROOT, "include", "fpng_amd.h")).read()
    for name in ("fpng_amd_decode_batch_png", "fpng_amd_decode_batch_device_png", "fpng_amd_decode_png_last_kernel_ms"):
        assert getattr(lib, name) is not None
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
    assert re.search(r"#define FPNG_AMD_DECODE_UNSUPPORTED_PNG 67\b", hdr) and re.search(r"#define FPNG_AMD_PNG_GENERAL_ONLY 1u\b", hdr)
    assert re.search(r"#define FPNG_AMD_ABI_VERSION 5\b", hdr)
    import fpng_amd
    assert fpng_amd.FPNG_AMD_DECODE_UNSUPPORTED_PNG == 67 and fpng_amd.FPNG_AMD_PNG_GENERAL_ONLY == 1
    assert hasattr(fpng_amd.Encoder, "decode_device_png") and hasattr(fpng_amd.Encoder, "decode_batch_png")
