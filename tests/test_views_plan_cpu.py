"""No-GPU tests of the views calls' host plumbing: which C entry point a descriptor goes through and with which arguments
(fpng_amd.api.views_entry, for every combination of stages, both layouts, files in host and in device memory), and the record
building of the view plan (fpng_amd/csrc/view_plan.h) as a stand-alone program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import itertools
import os
import subprocess

import pytest

from fpng_amd import _lib
from fpng_amd.api import DecodeBatchMultiView, DecodeBatchMultiViewHwc, views_entry

STAGES = ("colors", "posts", "warps", "tones", "enhances")  # colour < post < warp < tone < enhance
SUFFIXES = ("", "_color", "_post", "_warp", "_tone", "_enhance")
RECORDS = (_lib.ViewColor, _lib.ViewPost, _lib.ViewWarp, _lib.ViewTone, _lib.ViewEnhance)


@pytest.mark.parametrize("device_data", [False, True])
@pytest.mark.parametrize("layout", ["planar", "hwc"])
def test_entry_point_choice(built_lib, layout, device_data):
    """the last present stage names the call, and the call takes the record arrays of all stages up to it -- present or None"""
    lib = _lib.load()
    cls, dest = (DecodeBatchMultiView, _lib.ViewDest) if layout == "planar" else (DecodeBatchMultiViewHwc, _lib.ViewDestHwc)
    for present in itertools.product([False, True], repeat=5):
        for fmt in (None, _lib.FloatFormat()):
            batch = cls([b""], [[None]], (_lib.PngPlanarIn * 1)(), (_lib.DecodeResult * 1)(), device_data, [], (C.c_uint32 * 1)(1), (_lib.Crop * 1)(),
                        (_lib.ResizeView * 1)(), (dest * 1)(), fmt)
            for name, rec, there in zip(STAGES, RECORDS, present):
                if there:
                    setattr(batch, name, (rec * 1)())
            last = max((k + 1 for k in range(5) if present[k]), default=0)
            symbol, args = views_entry(layout, device_data, batch)
            assert symbol == f"fpng_amd_decode_batch{'_device' if device_data else ''}_{layout}_views{SUFFIXES[last]}", (present, symbol)
            assert len(args) == 8 + last and args[:6] == [batch.arr, 1, batch.counts, batch.crops, batch.views, batch.dests] and args[-1] is batch.res
            for k in range(last):
                assert args[6 + k] is getattr(batch, STAGES[k]) and (args[6 + k] is None) == (not present[k]), (present, k)
            assert (args[-2] is None) == (fmt is None)
            # the symbol is in the library, with a parameter for the encoder and one for each of these
            fn = getattr(lib, symbol)
            assert len(_lib.SIGNATURES[symbol][1]) == len(args) + 1 == len(fn.argtypes)
            assert fn.argtypes[7:7 + last] == [C.POINTER(r) for r in RECORDS[:last]] and fn.argtypes[6] == C.POINTER(dest)


def test_the_view_plan_under_the_sanitizers(built_lib, tmp_path):
    """tests/cpp/view_plan_build.cpp, a stand-alone program over view_plan.h -- the plan's records for four files with 2, 1, 3 and 1
    views, the second without a job, through the set-up block, for both layouts and the plain, colour and post families -- built with
    the address and undefined-behaviour sanitizers and run on the CPU: every check of the index arrays holds and there is no report"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "view_plan_build")
    # (the kernels' headers name HIP's stream type: the HIP headers are on the include path, the runtime is not linked.
    #  -Wno-unknown-pragmas: the headers' `#pragma clang fp contract`.  The sanitizers' runtimes are linked into the program where the
    #  compiler has them as archives, so that it starts in any environment)
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cmd = ["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(root, "fpng_amd", "csrc"),
           "-I", os.path.join(root, "include"), "-I", os.path.join(rocm, "include"), os.path.join(root, "tests", "cpp", "view_plan_build.cpp"), "-o", exe]
    r = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if r.returncode != 0:
        r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert run.returncode == 0 and not run.stderr, (run.returncode, run.stderr[-2000:])
    assert run.stdout.splitlines() == [f"ok {layout} {family}" for layout in ("planar", "hwc") for family in (0, 1, 5)] + ["ok empty"]
