"""No-GPU test of the rule that cuts a file into CRC ranges and folds their partials (fpng_amd/csrc/crc_geometry.h).

tests/cpp/crc_geometry.cpp, a stand-alone program over the header built with the address and undefined-behaviour sanitizers,
prints the rule for a grid of (span, n_jobs, crc_blocks); assemble_geometry.py, the same rule restated in Python from the header's
comment, must say the same line for line.  What held only by argument is asserted over the grid: a file never has more ranges than
its job's crc_blocks (the partials' slots: api.cpp sizes d_partials by it, and assemble_kernel's grid), every index into
CrcDeviceTables::fold lies inside fold[13][256], and a thread of the fold takes at most 2^8 partials."""
import hashlib
import json
import os
import subprocess

import pytest

import assemble_geometry as AG

N_JOBS = (1, 2, 7, 8, 9, 64, 511, 512, 513, 4096)
OFFSETS = (0, 1, 16, 64)
MAX_SPAN = 0xFFFFFFFF  # scan_kernel refuses a stored file past it, and a compressed one is smaller than its stored form (check_dims: < 4 GiB of filtered bytes)


def _grid():
    blocks = {2, 3, 4, 5, 6, 7, 70000}
    for p in range(3, 17):
        blocks |= {(1 << p) - 1, 1 << p, (1 << p) + 1}
    ms = {1, 2, 3, 4, 5}
    for p in range(3, 17):
        ms |= {(1 << p) - 1, 1 << p, (1 << p) + 1}
    spans = {64, 65, 80, 4095, MAX_SPAN, MAX_SPAN - 15, MAX_SPAN - 16}
    for e in range(12, 17):
        for m in ms:
            for d in OFFSETS:
                spans |= {m * (1 << e) + d, m * (1 << e) - d}
    spans = sorted(s for s in spans if 64 <= s <= MAX_SPAN)
    return [(s, n, b) for s in spans for n in N_JOBS for b in sorted(b for b in blocks if 2 <= b <= 70000)]


def _consistent(span, blocks):
    """the api's promise (fpng_amd_encode_submit: crc_blocks = ceil(max encoded size / 64 KiB) + 1): the file is no larger than the
    image's maximum size"""
    return span + 16 <= (blocks - 1) * 65536


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path_factory.mktemp("crc_geometry") / "crc_geometry")
    # (the sanitizers' runtimes are linked into the program where the compiler has them as archives, so that it starts in any environment)
    cmd = ["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", os.path.join(root, "fpng_amd", "csrc"),
           os.path.join(root, "tests", "cpp", "crc_geometry.cpp"), "-o", exe]
    r = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if r.returncode != 0:
        r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    grid = _grid()
    text = "".join("%d %d %d\n" % t for t in grid)
    env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([exe], input=text, capture_output=True, text=True, env=env, timeout=120)
    assert run.returncode == 0 and not run.stderr, (run.returncode, run.stderr[-2000:])
    out = run.stdout.splitlines()
    assert len(out) == len(grid)
    return grid, out


def test_the_rule_is_the_python_text(lines):
    grid, out = lines
    assert len(grid) > 100000
    seen_rl, seen_g = set(), set()
    for (span, n_jobs, blocks), ln in zip(grid, out):
        want = (span, n_jobs, blocks) + AG.rule(span, n_jobs, blocks)
        assert ln == " ".join(str(v) for v in want), (ln, want)
        rl, n_ranges, g, pad, sliver, step_row, group_row = want[3:]
        assert 12 <= rl <= 16 and 0 <= pad <= 15 and sliver % 16 == 0 and n_ranges >= 1
        assert g <= 8 and (1 << g) <= AG.FOLD_COLS, want
        assert 0 <= step_row < AG.FOLD_ROWS and 0 <= group_row < AG.FOLD_ROWS, want
        if _consistent(span, blocks):
            assert n_ranges <= blocks, want
            seen_rl.add(rl), seen_g.add(g)
    assert seen_rl == {12, 13, 14, 15, 16} and seen_g == set(range(9))


def test_the_model_of_a_stored_file():
    """assemble_geometry.stored_walk against a file of stored blocks built byte by byte here"""
    for w, h, c in ((5, 4096, 3), (64, 255, 4), (13, 1700, 3), (9, 2000, 4)):
        stride = w * c + 1
        stream = bytearray()
        for r in range(h):
            stream += b"\0" + bytes([(r + i) & 0xFF or 1 for i in range(w * c)])
        z = bytearray(b"\x78\x01")
        header_at, filter_at = [], []
        for k in range(0, len(stream), 65535):
            header_at.append(58 + len(z))
            z += b"\0" * 5
            for s in range(k, min(k + 65535, len(stream))):
                if s % stride == 0:
                    filter_at.append(58 + len(z))
                z.append(stream[s])
        size = 58 + len(z) + 4 + 16
        walk = AG.stored_walk(w, h, c)
        assert walk["size"] == size == AG.stored_size(w, h, c)
        assert [e["offset"] for e in walk["headers"]] == header_at
        assert walk["filter_piece_offsets"] == sorted({o % 16 for o in filter_at}) and walk["filters"]["offset"].tolist() == filter_at
        ea = walk["end_aligned"]
        assert ea % 16 == 0 and 0 <= ea - (size - 20) < 16
        for e in walk["headers"]:
            inside = set(range(e["offset"] + 1, e["offset"] + 5))
            assert e["straddles_piece"] == any(o % 16 == 0 for o in inside)
            assert e["straddles_row"] == any((ea - o) % 4096 == 0 for o in inside)
            assert e["straddles_range"] == any((ea - o) % (1 << walk["geometry"].rl) == 0 for o in inside)
        f = walk["filters"]
        assert f["in_piece"].tolist() == [o % 16 for o in filter_at] and f["in_row"].tolist() == [(o - ea) % 4096 for o in filter_at]
        assert f["in_range"].tolist() == [(o - ea) % (1 << walk["geometry"].rl) for o in filter_at]


def test_the_fixture_is_the_model_and_the_oracle():
    """tests/golden/geometry.json: every case's cell is the model's, and every case of less than 1 MiB raw encodes, with the C
    restatement of the reference (oracle/), to the recorded size and sha256"""
    from cpu_ref import oracle
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "geometry.json")) as f:
        fix = json.load(f)
    cases = [dict(zip(fix["fields"], row)) for row in fix["cases"]]
    assert len({k["name"] for k in cases}) == len(cases) > 200
    for flags in (0, 1, 2):
        assert sum(1 for k in cases if k["group"] == "A" and k["flags"] == flags) + fix["fillers"][str(flags)]["n"] == fix["group_a_jobs"] == AG.GROUP_A_JOBS
    assert AG.want_of(AG.GROUP_A_JOBS) == 4
    small = 0
    for k in cases:
        n_jobs = AG.GROUP_A_JOBS if k["group"] == "A" else 1
        assert list(AG.geometry(k["w"], k["h"], k["c"], k["size"], n_jobs)) == k["cell"], k["name"]
        if k["flags"] == 2:
            assert k["size"] == AG.stored_size(k["w"], k["h"], k["c"]), k["name"]
        if k["w"] * k["h"] * k["c"] < 1 << 20:
            png = oracle().encode(AG.case_image(k["w"], k["h"], k["c"], k["seed"], k["noise_pixels"]), k["w"], k["h"], k["c"], k["flags"])
            assert len(png) == k["size"] and hashlib.sha256(png).hexdigest() == k["sha256"], k["name"]
            small += 1
    assert small > 150
