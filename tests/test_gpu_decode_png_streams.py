"""The general decode tier's inflate on the GPU (-m gpu) against streams written token by token (tests/deflate_writer.py,
tests/inflate_cases.py): the edges of the tables, of the emit step and of the bit reader, the refusals that belong to them, and a
seeded random corpus of 300 streams, in the device form and the host form.  The host twin runs the lanes one after the other;
only here do 64 of them run at once.  Expectations are Pillow's pixels, which for these one-row grey files with filter byte 0 are
the writer's own bytes.  Every destination lies between guard bands (decode() of test_gpu_decode_png.py)."""
import functools
import os
import subprocess

import numpy as np
import pytest

import inflate_cases as ic
import png_cases as pc
from test_gpu_decode_png import ROOT, decode, enc  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu


@functools.lru_cache(None)
def pillow(name, desired):
    c = {c.name: c for c in ic.accepted_cases() + ic.random_cases() + list(ic.window_cases())}[name]
    exp = pc.expected(c.file, desired)
    if c.plain:  # (and Pillow's pixels are the bytes the writer meant)
        assert exp[0, :, 0].tobytes() == c.data[1:], name
    return exp


def check(enc, cases, desired, host):
    got = decode(enc, [c.file for c in cases], desired, host=host, dims=[c.dims for c in cases])
    for c, (st, px, chans) in zip(cases, got):
        assert st == 0, (c.name, st, host)
        assert chans == 1 and np.array_equal(px, pillow(c.name, desired)), (c.name, host)


@pytest.mark.parametrize("form", ["device", "host"])
def test_designed_streams(enc, form):
    """every designed accepted stream in one batch: status 0 and Pillow's pixels (4 channels in the device form, 3 in the host form)"""
    check(enc, ic.accepted_cases(), 4 if form == "device" else 3, form == "host")


@pytest.mark.parametrize("form", ["device", "host"])
def test_refused_streams(enc, form):
    cases = ic.refused_cases()
    got = decode(enc, [f for _, f, _ in cases], 4, host=form == "host", dims=[(8, 1)] * len(cases))
    for (name, _, want), (st, _, _) in zip(cases, got):
        assert st == want, (name, form)


def test_end_of_block_alone_and_its_unused_code(enc):
    good = [c for c in ic.accepted_cases() if c.name.startswith("eob_only")]
    bad = [f for n, f, _ in ic.refused_cases() if n == "eob_only_unused_code"]
    assert len(good) == 3 and len(bad) == 1
    for host in (False, True):
        got = decode(enc, [c.file for c in good] + bad, 4, host=host, dims=[c.dims for c in good] + [(8, 1)])
        for c, (st, px, _) in zip(good, got):
            assert st == 0 and np.array_equal(px, pillow(c.name, 4)), (c.name, host)
        assert got[-1][0] == pc.INVALID_IDAT


def test_declared_window_is_not_held_against_distances(enc):
    """documented leniency: a distance of 700 under a header that declares a 512-byte window is taken"""
    small, full = ic.window_cases()
    for host in (False, True):
        got = decode(enc, [small.file, full.file], 4, host=host, dims=[small.dims, full.dims])
        for st, px, _ in got:
            assert st == 0 and np.array_equal(px, pillow(full.name, 4)), host


def test_stream_that_ends_on_the_files_last_bit_equals_the_host_twin(enc, tmp_path):
    """parity only: the final end-of-block symbol's last bit is the last bit of the last IDAT byte and no Adler-32 follows"""
    exe = str(tmp_path / "png_inflate_host")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "fpng_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "png_inflate_host.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    c = ic.ends_on_last_bit_case()
    path = str(tmp_path / "lastbit.png")
    open(path, "wb").write(c.file)
    twin = subprocess.run([exe, "4", path], capture_output=True, text=True, check=True).stdout.split()
    for host in (False, True):
        (st, px, _), = decode(enc, [c.file], 4, host=host, dims=[c.dims])
        assert st == int(twin[0]), host
        if st == 0:
            assert pc.pixel_hash(px.tobytes()) == int(twin[4], 16), host


def test_random_streams(enc):
    """the 300 seeded streams in one batch, device form"""
    assert len(ic.random_cases()) >= 300
    check(enc, ic.random_cases(), 4, False)


def _groups(cases, limit):
    """how many groups the host form makes of the batch (include/fpng_amd.h: scanlines and file bytes, each rounded up to 256, count against the limit)"""
    groups, room = 0, 0
    for c in cases:
        need = (c.dims[0] + 1 + 255) // 256 * 256 + (len(c.file) + 255) // 256 * 256
        if not groups or room + need > limit:
            groups, room = groups + 1, 0
        room += need
    return groups


def test_random_streams_in_groups_host_form(enc):
    """the same batch from host memory under a scratch limit that takes four or more groups: the host form counts the files' own bytes
    against the limit too"""
    cases = ic.random_cases()
    total = sum((c.dims[0] + 1 + 255) // 256 * 256 + (len(c.file) + 255) // 256 * 256 for c in cases)
    limit = total // 4
    assert _groups(cases, limit) >= 4 and _groups(cases, 1 << 30) == 1
    os.environ["FPNG_AMD_PNG_SCRATCH_LIMIT"] = str(limit)
    try:
        check(enc, cases, 4, True)
    finally:
        del os.environ["FPNG_AMD_PNG_SCRATCH_LIMIT"]
