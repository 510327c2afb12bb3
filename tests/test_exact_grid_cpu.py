"""No-GPU tests of fpng_amd/csrc/exact_grid.h: the record search that the view-stage kernels run and the host's cut of a prefix array
into launches, which all seven exact-grid launchers go through.

A GPU test cannot reach the cut: a launch is split only past 2^24 - 1 workgroups.  tests/cpp/exact_grid.cpp, a stand-alone program
over the header built with the address and undefined-behaviour sanitizers, runs exact_grid_walk with a small limit (and with the
default one on prefixes near 2^32) and exact_grid_find / exact_grid_within for every workgroup of small prefix arrays; the rule
restated in Python says what the answers must be.

The walk checks every record before it launches anything: where it returns false, no piece has been launched (the loops it
replaces had launched the pieces in front of the record they refused)."""
import bisect
import os
import subprocess

import pytest

DEFAULT_LIMIT = (1 << 32) // 256 - 1  # a launch of 256-thread workgroups holds fewer than 2^32 threads


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path_factory.mktemp("exact_grid") / "exact_grid")
    # (the sanitizers' runtimes are linked into the program where the compiler has them as archives, so that it starts in any environment)
    cmd = ["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-I", os.path.join(root, "fpng_amd", "csrc"),
           os.path.join(root, "tests", "cpp", "exact_grid.cpp"), "-o", exe]
    r = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if r.returncode != 0:
        r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]

    def run(lines):
        env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
        out = subprocess.run([exe], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True, env=env, timeout=60)
        assert out.returncode == 0 and not out.stderr, (out.returncode, out.stderr[-2000:])
        got = [[int(t) for t in ln.split()[1:]] for ln in out.stdout.splitlines()]
        assert len(got) == len(lines)
        return got
    return run


def _prefix(counts, first=0):
    pre = [first]
    for c in counts:
        pre.append(pre[-1] + c)
    return pre


def _walk_model(pre, limit):
    """(ok, pieces): refused where a record has no workgroups or more than the limit, and then nothing is launched; else the greedy
    pieces (r0, r1, workgroups)"""
    n = len(pre) - 1
    if any(pre[k + 1] <= pre[k] or pre[k + 1] - pre[k] > limit for k in range(n)):
        return False, []
    pieces, r0 = [], 0
    while r0 < n:
        r1 = r0 + 1
        while r1 < n and pre[r1 + 1] - pre[r0] <= limit:
            r1 += 1
        pieces.append((r0, r1, pre[r1] - pre[r0]))
        r0 = r1
    return True, pieces


def _check_walk(program, cases, limit_arg, limit):
    got = program(["walk %d 256 %d %s" % (limit_arg, len(pre) - 1, " ".join(map(str, pre))) for pre in cases])
    for pre, g in zip(cases, got):
        n = len(pre) - 1
        ok, count, flat = g[0], g[1], g[2:]
        pieces = [tuple(flat[3 * k:3 * k + 3]) for k in range(count)]
        assert len(flat) == 3 * count
        want_ok, want = _walk_model(pre, limit)
        assert (bool(ok), pieces) == (want_ok, want), (pre, limit, g)
        if ok:  # the properties themselves, not only the model's word
            assert [p[0] for p in pieces] == [0] * (n > 0) + [p[1] for p in pieces[:-1]] and (not pieces or pieces[-1][1] == n)  # [0, n), in order, no gaps
            for r0, r1, groups in pieces:
                assert r1 > r0 and groups == pre[r1] - pre[r0] and 1 <= groups <= limit
                assert r1 == n or pre[r1 + 1] - pre[r0] > limit  # greedy: one more record would exceed the limit
        else:
            assert not pieces  # refused: nothing was launched


def test_the_walk_with_a_small_limit(program):
    """limit 7: no records, one record, every record exactly at the limit, one over it, a record without workgroups at the first, a
    middle and the last position (pre equal, and pre decreasing), mixed sizes, and a pre[0] that is not 0"""
    L = 7
    cases = [[0], [5], _prefix([1]), _prefix([L]), _prefix([L + 1]), _prefix([L] * 5), _prefix([L, L, L + 1, L]), _prefix([L + 1, 1, 1]), _prefix([1, 1, L + 1]),
             _prefix([0, 3, 2]), _prefix([3, 0, 2]), _prefix([3, 2, 0]), [0, 3, 2, 6], [4, 3, 9], [0, 3, 9, 8], _prefix([0]),
             _prefix([1] * 20), _prefix([3, 4, 1, 6, 2, 2, 2, 7, 1, 5, 3]), _prefix([6, 2, 5, 3, 4, 4], first=1000), _prefix([2] * 9, first=(1 << 40) + 3)]
    import random
    rng = random.Random(7)
    for _ in range(200):
        cases.append(_prefix([rng.randint(1, L) for _ in range(rng.randint(1, 30))], first=rng.choice([0, 11, 1 << 33])))
    for _ in range(50):  # one bad record somewhere
        counts = [rng.randint(1, L) for _ in range(rng.randint(1, 12))]
        counts[rng.randrange(len(counts))] = rng.choice([0, L + 1, L + 100])
        cases.append(_prefix(counts))
    _check_walk(program, cases, L, L)
    assert sum(_walk_model(pre, L)[0] for pre in cases) > 200 and sum(not _walk_model(pre, L)[0] for pre in cases) > 50


def test_the_walk_with_the_default_limit(program):
    """the launchers' own limit, 2^24 - 1 workgroups of 256 threads: prefix values near and past 2^32, where the differences need 64 bits"""
    assert program(["limit 256", "limit 64"]) == [[DEFAULT_LIMIT], [(1 << 32) // 64 - 1]]
    D = DEFAULT_LIMIT
    cases = [_prefix([D]), _prefix([D + 1]), _prefix([D, D, D]), _prefix([D - 1, 1, 1, D - 1, 2]), _prefix([1, D]), _prefix([D, 1]),
             _prefix([5, 6], first=(1 << 32) - 7), _prefix([D, D], first=(1 << 32) - D - 3), _prefix([1 << 32]), _prefix([3, (1 << 32) + 3, 3]),
             _prefix([D // 2 + 1] * 7, first=(1 << 32) - 1), _prefix([1000] * 40, first=(1 << 32) - 20000), [1 << 32, (1 << 32) + 5, 4], _prefix([D] * 300)]
    _check_walk(program, cases, 0, D)


def test_the_search_finds_every_workgroup(program):
    """for strictly increasing prefix arrays of 1 .. 70 records, counts of 1, 2, mixed and large, pre[0] zero or not (a launch's
    second piece): every workgroup b of the launch belongs to the record lo with pre[lo] <= pre[0] + b < pre[lo + 1], at g - pre[lo]"""
    import random
    rng = random.Random(70)
    cases = []
    for n in list(range(1, 20)) + [31, 32, 33, 63, 64, 65, 70]:
        for first in (0, 12345, (1 << 32) - 5):
            cases += [_prefix([1] * n, first), _prefix([2] * n, first), _prefix([rng.choice([1, 2, 3, 50]) for _ in range(n)], first)]
    cases += [_prefix([4000, 1, 1, 3000, 2], 99), _prefix([1, 5000], 0), _prefix([5000, 1], 1 << 40)]
    got = program(["find %d %s" % (len(pre) - 1, " ".join(map(str, pre))) for pre in cases])
    for pre, g in zip(cases, got):
        assert all(a < b for a, b in zip(pre, pre[1:]))
        count = pre[-1] - pre[0]
        assert g[0] == count and len(g) == 1 + 2 * count
        for b in range(count):
            lo = bisect.bisect_right(pre, pre[0] + b) - 1
            assert (g[1 + 2 * b], g[2 + 2 * b]) == (lo, pre[0] + b - pre[lo]), (pre, b)
            assert pre[lo] <= pre[0] + b < pre[lo + 1]
