"""The general decode tier's un-filter kernel and pixel expansion on the GPU (-m gpu) against the plain model of
tests/filter_writer.py, on the designed files of tests/unfilter_cases.py: predictor classes, dependency chains, shapes at the
edges of the 64-row bands and 64-step tiles, the kernel's own two refusals by position, the expansion table.  The CPU test
(test_png_unfilter_cpu.py) ties the model to Pillow and asserts what the files cover; the host twin runs the lanes one after the
other, only here do 64 of them run at once.  Every destination lies between guard bands (decode() of test_gpu_decode_png.py)."""
import os

import numpy as np
import pytest

import unfilter_cases as uc
from test_gpu_decode_png import decode, enc  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu


def check(enc, cases, desired, host=False):
    got = decode(enc, [c.file for c in cases], desired, host=host, dims=[c.dims for c in cases])
    for c, (st, px, chans) in zip(cases, got):
        assert st == 0, (c.name, st, host)
        assert np.array_equal(px, c.expected(desired)), (c.name, desired, host)
        assert chans == c.channels, (c.name, chans)
    return got


@pytest.mark.parametrize("form,desired", [("device", 3), ("device", 4), ("host", 4)])
def test_designed_files_give_the_models_pixels(enc, form, desired):
    """predictor classes, chains, shapes and the expansion table in one batch: status 0, the model's pixels, channels_in_file"""
    check(enc, uc.accepted_cases(), desired, form == "host")


@pytest.mark.parametrize("form", ["device", "host"])
def test_refusals_by_position(enc, form):
    """a filter byte of 5 / 255 in rows 0, 63, 64 and the last; a palette index equal to PLTE's entry count at the first and last
    pixel and in rows 63, 64, 129, with palettes of 1, 2, 10 and 255 entries: INVALID_IDAT each, next to the accepted files they
    differ from in one byte"""
    good, bad = uc.neighbour_cases(), uc.refusal_cases()
    cases = []
    for g in good:  # (each accepted file in front of its refusals)
        cases += [g] + [b for b in bad if b.neighbour == g.name]
    assert len(cases) == len(good) + len(bad)
    got = decode(enc, [c.file for c in cases], 4, host=form == "host", dims=[c.dims for c in cases])
    for c, (st, px, chans) in zip(cases, got):
        assert st == c.status, (c.name, st)
        if not c.status:
            assert np.array_equal(px, c.expected(4)) and chans == c.channels, c.name


@pytest.mark.parametrize("form", ["device", "host"])
def test_parity_only_files(enc, form):
    """a palette tRNS of 257 bytes, a grey tRNS of 1 byte, an RGB tRNS of 4 bytes: Pillow refuses them, the tier takes them as the
    model and the host twin do (include/fpng_amd.h)"""
    cases = uc.parity_cases()
    assert len(cases) == 3
    for desired in (3, 4):
        check(enc, cases, desired, form == "host")


def test_shapes_one_file_a_group(enc):
    """a scratch limit below any file's scanlines: every file is a group of its own, the scratch is reused 21 times"""
    cases = uc.shape_cases()
    assert min(len(c.scan) for c in cases) > 256
    one = check(enc, cases, 4)
    os.environ["FPNG_AMD_PNG_SCRATCH_LIMIT"] = "256"
    try:
        each = check(enc, cases, 4)
    finally:
        del os.environ["FPNG_AMD_PNG_SCRATCH_LIMIT"]
    for c, a, b in zip(cases, one, each):
        assert np.array_equal(a[1], b[1]), c.name
