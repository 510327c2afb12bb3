"""No-GPU tests of the PNG views call's door (fpng_amd_decode_batch(_device)_png_views): the symbols and the request record; the
Python entry function png_views_entry; the request's own refusals; that the call, without an encoder, refuses what the views call
of the request's family refuses -- the same code and the same message, case by case of test_views_refusals_cpu.py; and the request
gather (fpng_amd/csrc/png_views_gather.h) as a stand-alone program, plainly and under the sanitizers."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

import fpng_amd
from fpng_amd import _lib
from fpng_amd.api import Encoder, png_views_entry

import test_views_refusals_cpu as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGE_ATTRS = ("colors", "posts", "warps", "tones", "enhances", "alphas", "resamples")


def test_symbols_record_and_exports(built_lib):
    """added after ABI version 5 without changing it: found with dlsym, declared in the header, bound by the package"""
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "fpng_amd.h")).read()
    for name in ("fpng_amd_decode_batch_png_views", "fpng_amd_decode_batch_device_png_views"):
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
    assert re.search(r"#define FPNG_AMD_DECODE_PNG_CROP_OUTSIDE 68\b", hdr) and re.search(r"#define FPNG_AMD_ABI_VERSION 5\b", hdr)
    assert lib.fpng_amd_abi_version() == 5
    assert fpng_amd.FPNG_AMD_DECODE_PNG_CROP_OUTSIDE == 68 and fpng_amd.FPNG_AMD_DECODE_UNSUPPORTED_PNG == 67
    assert C.sizeof(_lib.PngViews) == 112
    assert [n for n, _ in _lib.PngViews._fields_] == ["view_count", "crops", "views", "dests", "hwc", "fmt", *STAGE_ATTRS, "flags", "reserved"]
    assert _lib.PngViews.colors.offset == 48 and _lib.PngViews.flags.offset == 104 and _lib.PngViews.reserved.offset == 108
    for m in ("decode_device_png_views", "decode_batch_png_views", "make_decode_batch_png_views"):
        assert hasattr(Encoder, m)
    for out_of_scope in ("YUV destinations", "one view per file", "16-bit, 1/2/4-bit and interlaced", "png_inflate_kernel"):
        assert out_of_scope in hdr


def _address(p):
    return C.cast(p, C.c_void_p).value


@pytest.mark.parametrize("layout", ["planar", "hwc"])
@pytest.mark.parametrize("device_data", [False, True])
def test_png_views_entry_names_the_call_and_fills_the_request(layout, device_data):
    hwc = layout == "hwc"
    pngs = [b"x" * 8, b"y" * 8]
    crops = [[(0, 0, 8, 8), (1, 1, 4, 4)], [(0, 0, 8, 8)]]
    kw = dict(color=[[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], post=fpng_amd.view_post(solarize=100), warp=fpng_amd.view_warp(), tone=fpng_amd.view_tone(equalize=True),
              enhance=fpng_amd.view_enhance(color=0.5), alpha=fpng_amd.view_alpha("premultiplied"), resample="box")
    keys = list(kw)
    for dtype in (torch.uint8, torch.float16):
        outs = [[torch.empty((4, 4, 3) if hwc else (3, 4, 4), dtype=dtype) for _ in cs] for cs in crops]
        for last in range(len(keys) + 1):  # (each last-given stage, alone and with one stage in front of it)
            for given in ({keys[last - 1]} if last else set(), set(keys[max(0, last - 2):last])):
                db = Encoder.make_decode_batch_png_views(pngs, crops, outs, (4, 4), layout=layout, flags=last & 1, **{k: kw[k] for k in given})
                assert isinstance(db, fpng_amd.DecodeBatchPngViewsHwc if hwc else fpng_amd.DecodeBatchPngViews) and db.flags == (last & 1)
                symbol, args = png_views_entry(layout, device_data, db, db.flags)
                assert symbol == ("fpng_amd_decode_batch_device_png_views" if device_data else "fpng_amd_decode_batch_png_views")
                assert args[0] is db.arr and args[1] == 2 and args[3] is db.res and len(args) == 4
                rq = args[2]._obj
                assert isinstance(rq, _lib.PngViews) and (rq.flags, rq.reserved) == (last & 1, 0)
                assert _address(rq.view_count) == C.addressof(db.counts) and _address(rq.crops) == C.addressof(db.crops) and _address(rq.views) == C.addressof(db.views)
                assert _address(rq.hwc if hwc else rq.dests) == C.addressof(db.dests) and not (rq.dests if hwc else rq.hwc)
                assert (_address(rq.fmt) == C.addressof(db.fmt)) if dtype is torch.float16 else not rq.fmt
                for key, attr in zip(keys, STAGE_ATTRS):
                    if key in given:
                        assert _address(getattr(rq, attr)) == C.addressof(getattr(db, attr)), attr
                    else:
                        assert not getattr(rq, attr) and getattr(db, attr) is None, attr
    with pytest.raises(ValueError):
        Encoder.make_decode_batch_png_views(pngs, crops, outs, (4, 4), layout="chw")


def _request(a, hwc, stages, flags=0, reserved=0):
    rq = _lib.PngViews()
    for name in ("view_count", "crops", "views"):
        if a[name] is not None:
            setattr(rq, name, a[name])
    if a["dests"] is not None:
        setattr(rq, "hwc" if hwc else "dests", a["dests"])
    if a["fmt"] is not None:
        rq.fmt = C.pointer(a["fmt"])
    for s in stages:
        if a[s] is not None:
            setattr(rq, s, a[s])
    rq.flags, rq.reserved = flags, reserved
    return rq


def _call(name, files, rq, results):
    lib = _lib.load()
    rc = getattr(lib, name)(None, files, 2, C.byref(rq) if rq is not None else None, results)
    return rc, lib.fpng_amd_last_error().decode()


@pytest.mark.parametrize("name", ["fpng_amd_decode_batch_png_views", "fpng_amd_decode_batch_device_png_views"])
@pytest.mark.parametrize("layout", ["planar", "hwc"])
def test_the_requests_own_refusals_come_first(built_lib, name, layout):
    """a NULL request, reserved != 0, unknown flags, both or neither of dests / hwc: FPNG_AMD_ERR_INVALID_ARG before an encoder is
    needed, and before anything the family's call would refuse"""
    hwc = layout == "hwc"
    a = R._good(hwc)
    R.FAULTS["bad_post"][1](a)  # (a fault of the family's own: reported only behind the request's)
    assert _call(name, a["files"], None, a["results"]) == (-1, "null request")
    assert _call(name, a["files"], _request(a, hwc, R.STAGES, reserved=1), a["results"]) == (-1, "fpng_amd_png_views::reserved must be 0")
    for flags in (2, 3, 1 << 31):
        assert _call(name, a["files"], _request(a, hwc, R.STAGES, flags=flags), a["results"]) == (-1, "unknown fpng_amd_png_views::flags bits (FPNG_AMD_PNG_GENERAL_ONLY)")
    both = _request(a, hwc, R.STAGES)
    other = R._good(not hwc)
    setattr(both, "dests" if hwc else "hwc", other["dests"])
    assert _call(name, a["files"], both, a["results"]) == (-1, "exactly one of fpng_amd_png_views::dests and hwc")
    neither = _request(dict(a, dests=None), hwc, R.STAGES)
    assert _call(name, a["files"], neither, a["results"]) == (-1, "exactly one of fpng_amd_png_views::dests and hwc")
    assert _call(name, a["files"], _request(a, hwc, R.STAGES, flags=1), a["results"]) == (-1, R.BAD_POST)


@pytest.mark.parametrize("name", ["fpng_amd_decode_batch_png_views", "fpng_amd_decode_batch_device_png_views"])
@pytest.mark.parametrize("layout", ["planar", "hwc"])
def test_the_call_refuses_what_its_familys_views_call_refuses(built_lib, name, layout):
    """every case of test_views_refusals_cpu.py, for every family: the request is judged as the views call whose last array is the last
    stage array that is given -- the code and the exact message of that call on the same arrays (its own table says what they are)"""
    hwc = layout == "hwc"
    dev = "_device" if "_device_" in name else ""
    ran = 0
    for k in range(len(R.FAMILIES)):
        for case in R.CASES:
            if not R._applies(case, layout, k) or "null_dests" in case:  # (neither dests nor hwc: the request's own refusal, above)
                continue
            a = R._good(hwc)
            for f in case:
                R.FAULTS[f][1](a)
            given = [s for s in R.STAGES[:k] if a[s] is not None]
            family = max((R.STAGES.index(s) + 1 for s in given), default=0)
            twin = f"fpng_amd_decode_batch{dev}_{layout}_views{R.FAMILIES[family]}"
            lib = _lib.load()
            fmt = C.byref(a["fmt"]) if a["fmt"] is not None else None
            rc = getattr(lib, twin)(None, a["files"], 2, a["view_count"], a["crops"], a["views"], a["dests"], *[a[s] for s in R.STAGES[:family]], fmt, a["results"])
            want = (rc, lib.fpng_amd_last_error().decode())
            if family == k:  # (no stage array was taken away: the table's own expectation for that call)
                assert want == (-1, R.expected(twin, case)), (twin, case)
            got = _call(name, a["files"], _request(a, hwc, R.STAGES[:k]), a["results"])
            assert got == want, (k, case, got, want)
            ran += 1
    assert ran >= 200
    a = R._good(hwc)
    assert _call(name, a["files"], _request(a, hwc, R.STAGES), a["results"]) == (-1, "null/empty batch")  # (the good set: only the missing encoder stops it)


@pytest.mark.parametrize("which", ["plain", "sanitizers"])
def test_the_request_gather(tmp_path, which):
    """files {1, 3} of a 5-file request with 2, 1, 3, 1, 2 views and every array given, compacted: a stand-alone program over
    png_views_gather.h, which the host compiler builds alone"""
    exe = str(tmp_path / "png_views_gather_host")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "fpng_amd", "csrc"),
           os.path.join(ROOT, "tests", "cpp", "png_views_gather_host.cpp"), "-o", exe]
    if which == "sanitizers":
        cmd += ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert (r.returncode, r.stdout, r.stderr) == (0, "ok\n", "")
