"""No-GPU test of the general decode tier's host rules (fpng_amd/csrc/png_tier_plan.h), which fpng_amd_decode_batch(_device)_png and
_png_views share: the grouping rule, the scratch layout, the kernels' file records, what counts as an fpng file and the fold of a
file's state into its result -- a stand-alone program (tests/cpp/png_tier_plan_host.cpp) over the header, which the host compiler
builds alone, plainly and under the sanitizers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("which", ["plain", "sanitizers"])
def test_the_tier_plan(tmp_path, which):
    exe = str(tmp_path / "png_tier_plan_host")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "fpng_amd", "csrc"),
           os.path.join(ROOT, "tests", "cpp", "png_tier_plan_host.cpp"), "-o", exe]
    if which == "sanitizers":
        cmd += ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert (r.returncode, r.stdout, r.stderr) == (0, "ok\n", "")

