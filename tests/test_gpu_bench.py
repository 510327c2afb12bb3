"""bench.py on the GPU: a plain run times the steps and prints the headline alone; --full adds the golden-vector parity check, the
roofline and the `decode` object (and, without --no-cpu-baseline, the CPU baselines and end_to_end)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--workload", "512", "--batch", "4", "--steps", "3", "--warmup", "1", "--prewarm", "2", "--decode-steps", "2"]


def _line(args):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_prints_the_headline_alone():
    line = _line(SMALL)
    assert line["value"] > 0 and line["ms_per_step"] > 0 and line["unit"] == "MP/s" and line["higher_is_better"] is True
    assert line["steps"] == 3 and line["warmup"] == 1 and line["config"]["batch_per_gpu"] == 4
    assert not {"parity_checked", "roofline", "decode", "end_to_end", "cpu_baseline"} & set(line)


@pytest.mark.gpu
def test_full_run_adds_parity_roofline_and_decode():
    line = _line(SMALL + ["--full", "--no-cpu-baseline"])
    assert line["parity_checked"] is True and line["parity_images"] == 1  # (tests/golden/kat.json holds image 0 of this set)
    assert line["roofline"]["kernel"].endswith("_kernel") and line["roofline"]["phase_ms"]
    assert line["decode"]["parity_checked"] is True and line["decode"]["steps"] == 2
    assert "cpu_baseline" not in line and "end_to_end" not in line
