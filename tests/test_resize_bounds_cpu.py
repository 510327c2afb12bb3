"""No-GPU tests of what the resize kernels' LDS layout rests on, and of the model the GPU tests of full tiles take their bytes from.

resize_max_taps, resize_tile_rows and resize_tile_lds (fpng_amd/csrc/resize.h) are the host's promises to dec_resize_tile,
dec_resize_hwc_kernel and dec_resize_color_kernel: a tile's weights fit taps x 64 and taps x 16 dwords, and the source rows that 16
consecutive output rows reach fit the T buffer's `rows` rows.  The kernels clamp where a promise would not hold (`nrows = min(..,
r.rows)`, the cap of resize_weights_of), so a bound that is one short gives wrong bytes with status 0 and no fault.  They are not in
the ABI: tests/cpp/resize_bounds.cpp, a stand-alone program over resize.h built with the address and undefined-behaviour sanitizers,
prints them next to what resize_taps_of / resize_source_span really need, and the rule restated in Python says what that must be.

The second test pins resize_view_model.resize_plane to Pillow at the scale limits, where test_gpu_resize_limits.py uses it."""
import os
import subprocess

import numpy as np
import pytest

import resize_limit_views as LV
import resize_view_model as VM

FILTERS = {"bilinear": 0, "bicubic": 1}
TILE_W, TILE_H = 64, 16  # kResizeTileW, kResizeTileH
# recorded values of the current formulas (tile 64 x 16, taps <= 65, rows = ceil((15 + 2 s_f) * scale) + 3): a change to the tile's
# size or to a bound has to touch them knowingly.  Bilinear: 32 x in both axes, 65 taps and 547 rows; bicubic: 16 x, 65 and 307
MOST_LDS = {"bilinear": 56448, "bicubic": 41088}


def _first_end(in_size, out_size, filter):
    """first[o] and first[o] + count[o] of resize_view_model.axis_weights for every o, without the weights: the rule's own lines in
    float64 arrays (the same IEEE operations in the same order; np.trunc is int()'s truncation toward zero).  axis_weights computes
    every weight in Python and takes a minute over the pairs below; test_the_bounds_hold holds this against it where it is affordable"""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = VM.SUPPORT[filter] * fs
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    first = np.maximum(np.trunc(center - support + 0.5), 0.0).astype(np.int64)
    end = np.minimum(np.trunc(center + support + 0.5), float(in_size)).astype(np.int64)
    return first, end


def _needs(in_size, out_size, filter, first=None, end=None):
    """(the most taps of a sample, the most source samples that min(16, out) consecutive samples reach)"""
    if first is None:
        first, end = _first_end(in_size, out_size, filter)
    n = min(TILE_H, out_size)
    return int((end - first).max()), int((end[n - 1:] - first[:out_size - n + 1]).max())


def _pairs():
    pairs = set(LV.axis_pairs())
    for f in VM.FILTERS:
        limit = VM.MAX_SCALE[f]
        pairs |= {(f, i, o) for o in range(1, 41) for i in range(1, limit * o + 1)}               # every `in` inside the limit
        pairs |= {(f, limit * o - d, o) for o in range(1, 131) for d in range(41) if limit * o - d >= 1}  # the limit and the 40 below it
        pairs |= {(f, k, k) for k in (1, 2, 15, 16, 17, 63, 64, 65, 600, 2080, 4096)}               # in == out
        pairs |= {(f, 1, o) for o in (1, 2, 16, 17, 65, 224, 4096)}                                  # in == 1
        pairs |= {(f, i, 1) for i in range(1, limit + 1)}                                            # out == 1
    return sorted(pairs)


def _pinned(pairs):
    """the pairs at which _first_end is held against axis_weights itself: what the GPU tests resize with (but the 4096-sample axes),
    every pair with out <= 10, the limit and the two below it for every fifth out, in == out, in == 1"""
    gpu = LV.axis_pairs()
    return [(f, i, o) for f, i, o in pairs
            if ((f, i, o) in gpu and o <= 300) or o <= 10 or (o % 5 == 0 and i >= VM.MAX_SCALE[f] * o - 2) or (i == o and o <= 65) or (i == 1 and o <= 224)]


@pytest.fixture(scope="module")
def bounds(tmp_path_factory):
    """the program's lines for _pairs(): {(filter, in, out): (taps, rows, lds, count, span)}"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path_factory.mktemp("resize_bounds") / "resize_bounds")
    # (-Wno-unknown-pragmas: the header's `#pragma clang fp contract`; g++ in ISO mode does not contract on x86-64.  The sanitizers'
    #  runtimes are linked into the program where the compiler has them as archives, so that it starts in any environment)
    cmd = ["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-I", os.path.join(root, "fpng_amd", "csrc"),
           os.path.join(root, "tests", "cpp", "resize_bounds.cpp"), "-o", exe]
    r = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if r.returncode != 0:
        r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    pairs = _pairs()
    text = "".join("%d %d %d\n" % (FILTERS[f], i, o) for f, i, o in pairs)
    env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([exe], input=text, capture_output=True, text=True, env=env, timeout=120)
    assert run.returncode == 0 and not run.stderr, (run.returncode, run.stderr[-2000:])
    names = {v: k for k, v in FILTERS.items()}
    out = {}
    for ln in run.stdout.splitlines():
        v = [int(t) for t in ln.split()]
        assert len(v) == 8, ln
        out[(names[v[0]], v[1], v[2])] = tuple(v[3:])
    assert sorted(out) == pairs  # (a line for every pair: none refused, none dropped)
    return out


def test_the_bounds_hold(bounds):
    """for every pair: the most taps of a sample is what the rule says and at most resize_max_taps; the most source rows under 16
    consecutive samples is what the rule says and at most resize_tile_rows, which is at most `in`; the tile's LDS fits 64 KiB and
    holds the colour kernel's four row buffers (4 x (64 * C * E bytes, and 4 more where E < 4) in the place of the weights,
    inside max(resize_tile_lds, 16 * 64 * C))"""
    pairs = sorted(bounds)
    assert len(pairs) > 40000
    pinned = _pinned(pairs)
    assert len(pinned) > 2500 and LV.axis_pairs() - set(pinned) == {("bilinear", 600, 4096), ("bilinear", 130, 1792)}
    for f, i, o in pinned:
        mf, mc, _ = VM.axis_weights.__wrapped__(i, o, f)  # (not through the cache: nothing else asks for these)
        first, end = _first_end(i, o, f)
        assert first.tolist() == mf and (end - first).tolist() == mc, (f, i, o)
        assert _needs(i, o, f) == (max(mc), max(VM.axis_span(i, o, o0, min(TILE_H, o), f)[1] - VM.axis_span(i, o, o0, min(TILE_H, o), f)[0] for o0 in range(o - min(TILE_H, o) + 1)))
    most = {f: 0 for f in VM.FILTERS}
    slack = 1 << 30
    for (f, i, o), (taps, rows, lds, count, span) in bounds.items():
        want = _needs(i, o, f)
        assert (count, span) == want, (f, i, o, (count, span), want)
        assert 1 <= count <= taps <= VM.MAX_TAPS, (f, i, o, count, taps)
        assert 1 <= span <= rows <= i, (f, i, o, span, rows)
        assert lds == (taps * TILE_W + taps * TILE_H + 2 * (TILE_W + TILE_H)) * 4 + rows * TILE_W and lds <= 65536, (f, i, o, lds)
        for c in (3, 4):
            for e in (1, 2, 4):
                assert max(lds, TILE_H * TILE_W * c) >= 4 * (TILE_W * c * e + (4 if e < 4 else 0)), (f, i, o, c, e)
        most[f] = max(most[f], lds)
        if rows < i:
            slack = min(slack, rows - span)
    print("largest resize_tile_lds:", most, "least rows - span where rows < in:", slack)
    assert most == MOST_LDS
    for f in VM.FILTERS:  # (both maxima are the scale limit's)
        limit = VM.MAX_SCALE[f]
        assert bounds[(f, limit * 24, 24)][2] == MOST_LDS[f], f


# (source (w, h), output (w, h), filter): full tiles just under the scale limits and exactly at them
PILLOW_PAIRS = [((95, 1055), (3, 33), "bilinear"), ((95, 527), (6, 33), "bicubic"), ((2075, 61), (65, 2), "bilinear"), ((1037, 61), (65, 4), "bicubic"),
                ((2080, 768), (65, 24), "bilinear"),
                ((96, 1056), (3, 33), "bilinear"), ((96, 528), (6, 33), "bicubic"), ((2080, 64), (65, 2), "bilinear"), ((1040, 64), (65, 4), "bicubic")]


def test_the_model_is_pillow_at_the_scale_limits():
    """resize_view_model.resize_plane == Image.resize byte for byte on seeded noise at 32 x (bilinear) and 16 x (bicubic) and just
    under: 65 taps a sample in one or both passes, where test_gpu_resize_limits.py takes its expected bytes from the model"""
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(2080)
    pil = {"bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC}
    most = 0
    for (w, h), (ow, oh), f in PILLOW_PAIRS:
        assert w <= VM.MAX_SCALE[f] * ow and h <= VM.MAX_SCALE[f] * oh
        most = max(most, max(VM.axis_weights(w, ow, f)[1]), max(VM.axis_weights(h, oh, f)[1]))
        p = rng.integers(0, 256, (h, w), dtype=np.uint8)
        want = np.asarray(Image.fromarray(p, "L").resize((ow, oh), pil[f]))
        got = VM.resize_plane(p, ow, oh, f)
        assert got.shape == (oh, ow) and np.array_equal(got, want), ((w, h), (ow, oh), f, int((got != want).sum()))
    assert most == VM.MAX_TAPS - 1  # (64 taps a sample at exactly 32 x and 16 x)


def _tile_model(p, full, window, filter, short):
    """dec_resize_tile's two passes restated tile by tile for one plane p (h, w) -> the window's (wh, ww) bytes, with a T buffer of
    (the rows the tile's 16 output rows reach) - short rows: short = 0 is the kernel with a bound that holds, short = 1 the kernel
    whose `nrows = min(.., r.rows)` drops the tile's last source row"""
    x, y, ww, wh = (0, 0) + tuple(full) if window is None else window
    t = VM.one_pass(p, full[0], filter)[:, x:x + ww]  # the horizontal pass: every source row, the window's columns
    first, count, K = VM.axis_weights(p.shape[0], full[1], filter)
    out = np.empty((wh, ww), dtype=np.uint8)
    for q0 in range(0, wh, TILE_H):
        rows = range(y + q0, y + min(q0 + TILE_H, wh))
        row0, nrows = first[rows[0]], first[rows[-1]] + count[rows[-1]] - first[rows[0]] - short
        for q in rows:
            f0 = first[q] - row0
            n = min(count[q], nrows - f0) if f0 < nrows else 0
            s = (1 << (VM.PRECISION_BITS - 1)) + (t[first[q]:first[q] + n].astype(np.int64) * np.asarray(K[q][:n], dtype=np.int64)[:, None]).sum(axis=0)
            out[q - y] = np.clip(s >> VM.PRECISION_BITS, 0, 255)
    return out


def test_a_t_buffer_one_row_short_would_be_seen():
    """why test_gpu_resize_limits.py's comparisons hold the kernels' `nrows = min(.., r.rows)` guard: for every view of LIMIT_VIEWS,
    on seeded noise, the tile model with a T buffer that holds its rows is the whole-image model, and with ONE row less its bytes
    differ in every view that shrinks rows -- a host bound one short of a tile's need gives wrong bytes there, and they are compared"""
    rng = np.random.default_rng(768)
    plane = rng.integers(0, 256, LV.LIMIT_FILE[::-1], dtype=np.uint8)
    seen = {}
    for crop, full, window, f in LV.LIMIT_VIEWS:
        p = plane[crop[1]:crop[1] + crop[3], crop[0]:crop[0] + crop[2]]
        x, y, w, h = (0, 0) + tuple(full) if window is None else window
        want = VM.resize_plane(p, full[0], full[1], f)[y:y + h, x:x + w]
        assert np.array_equal(_tile_model(p, full, window, f, 0), want), (crop, full, window, f)
        if crop[3] > full[1]:
            seen[(crop, full, window, f)] = int((_tile_model(p, full, window, f, 1) != want).sum())
    print("bytes that differ with a T buffer one row short:", seen)
    assert len(seen) == 9 and all(seen.values()), seen
