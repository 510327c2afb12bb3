"""The box un-filter of the PNG views call (fpng_amd/csrc/png_inflate_core.h: pngi_unfilter_box) on the CPU:
tests/cpp/png_unfilter_box_host.cpp runs pngi_inflate with only the box's rows kept and then the box walk, lane by lane, built plainly
and with -fsanitize=address,undefined (a stand-alone program, run as a child process).  Expectations are Pillow's pixels of the same
file, cropped and split into planes; for refusals, the status by where the damage lies relative to the box."""
import functools
import os
import subprocess

import numpy as np
import pytest

import filter_writer as fw
import png_cases as pc
import unfilter_cases as uc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CROP_OUTSIDE = 68


@pytest.fixture(scope="module")
def twins(tmp_path_factory):
    """(plain build, sanitizer build, a directory for the files)"""
    d = tmp_path_factory.mktemp("png_unfilter_box_host")
    src = os.path.join(ROOT, "tests", "cpp", "png_unfilter_box_host.cpp")
    base = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "fpng_amd", "csrc"), src]
    plain, san = str(d / "png_unfilter_box_host"), str(d / "png_unfilter_box_host_san")
    for exe, extra in ((plain, []), (san, ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DPNGI_GUARD=0"])):
        r = subprocess.run(base + extra + ["-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
    return plain, san, d


class Files:
    """files written once into the directory, named by their index"""

    def __init__(self, d, tag, files):
        self.paths = []
        for i, f in enumerate(files):
            p = str(d / f"{tag}_{i}.png")
            if not os.path.exists(p):
                with open(p, "wb") as fh:
                    fh.write(f)
            self.paths.append(p)


def run_box(exe, paths, planes, box):
    """-> [(status, hash, guard)] per file; any sanitizer report fails the run (non-zero exit, stderr)"""
    r = subprocess.run([exe, str(planes)] + [str(v) for v in box] + list(paths), capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.returncode, box, r.stderr[-3000:])
    lines = r.stdout.splitlines()
    assert len(lines) == len(paths)
    return [(int(a), int(h, 16), int(g)) for a, h, g in (ln.split() for ln in lines)]


@functools.lru_cache(None)
def pillow_rgba(file):
    return pc.expected(file, 4)


def planes_hash(file, planes, box):
    """the hash of Pillow's pixels of the file, cropped to the box, as `planes` tight planes"""
    x, y, w, h = box
    px = pillow_rgba(file)[y:y + h, x:x + w, :planes]
    return pc.pixel_hash(np.ascontiguousarray(px.transpose(2, 0, 1)).tobytes())


# ---- the boxes: every edge the walk has ----
YS, Y1S = (0, 63, 64, 65), (1, 64, 65, 128, 129)
XS, X1S = (0, 63, 64), (1, 64, 65)


def edge_boxes(w, h):
    """y in YS and y1 in Y1S + (h,), x in XS and x1 in X1S + (w,), every pair that is a box of the image; the 1 x 1 boxes in the four
    corners and at (63, 63) and (64, 64); the whole image"""
    rows = sorted({(y, y1) for y in YS for y1 in Y1S + (h,) if y < y1 <= h})
    cols = sorted({(x, x1) for x in XS for x1 in X1S + (w,) if x < x1 <= w})
    out = [(x, y, x1 - x, y1 - y) for y, y1 in rows for x, x1 in cols]
    out += [(x, y, 1, 1) for x, y in ((0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (63, 63), (64, 64)) if x < w and y < h]
    out.append((0, 0, w, h))
    return list(dict.fromkeys(out))


@functools.lru_cache(None)
def square_cases():
    """a 130 x 130 file per pixel size (and a palette file with a tRNS), every filter type somewhere in every band"""
    out = []
    for k, color in enumerate((0, 4, 2, 6, 3)):
        rng = np.random.default_rng(7000 + k)
        w = h = 130
        if color == 3:
            px = rng.integers(0, 256, (h, w), dtype=np.uint8)
            kw = dict(plte=uc._palette(7100), trns=bytes((3 + 41 * i) & 255 for i in range(200)))
        else:
            px, kw = uc._mix(rng, h, w * fw.BPP[color]), {}
        out.append(uc._from_pixels(f"square130_c{color}", w, h, color, px, [(y + k) % 5 for y in range(h)], **kw))
    return out


def test_edge_boxes_hold_what_the_issue_lists():
    boxes = edge_boxes(130, 130)
    assert {(b[1], b[1] + b[3]) for b in boxes} >= {(y, y1) for y in YS for y1 in Y1S + (130,) if y < y1}
    assert {(b[0], b[0] + b[2]) for b in boxes} >= {(x, x1) for x in XS for x1 in X1S + (130,) if x < x1}
    for b in ((0, 0, 1, 1), (129, 0, 1, 1), (0, 129, 1, 1), (129, 129, 1, 1), (63, 63, 1, 1), (64, 64, 1, 1), (0, 0, 130, 130)):
        assert b in boxes
    assert [fw.BPP[c.color] for c in square_cases()] == [1, 2, 3, 4, 1]


@pytest.mark.parametrize("which", ["plain", "sanitizers"])
def test_square_files_at_every_edge(twins, which):
    """the 130 x 130 files, every box of edge_boxes, both plane counts: Pillow's pixels, guards untouched"""
    plain, san, d = twins
    cases = square_cases()
    for c in cases:  # (Pillow agrees with the model on these files, as on unfilter_cases' own)
        assert np.array_equal(pillow_rgba(c.file), c.expected(4)), c.name
    files = Files(d, "square", [c.file for c in cases])
    for k, box in enumerate(edge_boxes(130, 130)):
        # (each build takes every box; the plane counts alternate, the other way round in the other build, and both for the whole image)
        for planes in ((3, 4) if box[2:] == (130, 130) else ((3, 4)[(k + (which == "plain")) % 2],)):
            got = run_box(plain if which == "plain" else san, files.paths, planes, box)
            for c, (status, hsh, guard) in zip(cases, got):
                assert status == 0 and guard == 1, (c.name, box, planes)
                assert hsh == planes_hash(c.file, planes, box), (c.name, box, planes)


def case_boxes(w, h):
    """of a designed file: the whole image, the corners, the band's and the tile's first and last pixel where the file has them,
    and a box whose far corner is inside"""
    out = [(0, 0, w, h)] + [(x, y, 1, 1) for x, y in ((0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (63, 63), (64, 64)) if x < w and y < h]
    out.append((min(63, w - 1), min(63, h - 1), min(2, w - min(63, w - 1)), min(2, h - min(63, h - 1))))
    out.append((w // 3, h // 3, max(1, w // 2), max(1, h // 2)))
    return list(dict.fromkeys(out))


@pytest.mark.parametrize("which", ["plain", "sanitizers"])
@pytest.mark.parametrize("planes", [3, 4])
def test_designed_files(twins, which, planes):
    """the accepted files of unfilter_cases.py (all five colour types, every filter, widths 127-130, 65 bands), grouped by size"""
    plain, san, d = twins
    by_dims = {}
    for c in uc.accepted_cases():
        by_dims.setdefault(c.dims, []).append(c)
    assert {c.color for c in uc.accepted_cases()} == {0, 2, 3, 4, 6}
    for (w, h), cases in by_dims.items():
        files = Files(d, f"designed_{w}x{h}", [c.file for c in cases])
        for box in case_boxes(w, h):
            got = run_box(plain if which == "plain" else san, files.paths, planes, box)
            for c, (status, hsh, guard) in zip(cases, got):
                assert status == 0 and guard == 1, (c.name, box)
                assert hsh == planes_hash(c.file, planes, box), (c.name, box)


def test_a_box_outside_runs_nothing(twins):
    plain, _, d = twins
    files = Files(d, "square", [c.file for c in square_cases()])
    for box in ((0, 0, 131, 1), (130, 0, 1, 1), (0, 130, 1, 1), (1, 1, 130, 130), (0, 0, 0, 5), (2 ** 32 - 1, 0, 2, 1)):
        assert run_box(plain, files.paths, 3, box) == [(CROP_OUTSIDE, 0, 1)] * len(files.paths)


@pytest.mark.parametrize("which", ["plain", "sanitizers"])
def test_refusals_by_where_the_box_lies(twins, which):
    """a filter byte above 4 in a visited row -- inside the box or above it -- refuses the file and below the box it does not; a
    palette index behind PLTE's count refuses the file inside the box only.  Where the file passes, the planes are Pillow's of the
    accepted neighbour: the one changed pixel lies outside the box and, by the files' design, changes no other pixel"""
    plain, san, d = twins
    exe = plain if which == "plain" else san
    good = {c.name: c for c in uc.neighbour_cases()}
    bad = {c.name: c for c in uc.refusal_cases()}
    w, seen = 70, set()
    # filter bytes: the 130-row file, rows 0, 63, 64 and 129
    for row in (0, 63, 64, 129):
        c = bad[f"filter_5_h130_row{row}"]
        files = Files(d, f"bad_{c.name}", [c.file])
        boxes = [(0, row, w, 1, "inside"), (10, row, 5, 1, "inside"), (69, 0, 1, 130, "inside")]
        if row:
            boxes += [(0, 0, w, row, "below"), (3, max(0, row - 2), 9, min(2, row), "below")]
        if row < 129:
            boxes += [(0, row + 1, w, 1, "above"), (20, row + 1, 3, 129 - row, "above")]
        for x, y, bw, bh, where in boxes:
            for planes in (3, 4):
                status, hsh, guard = run_box(exe, files.paths, planes, (x, y, bw, bh))[0]
                assert guard == 1
                if where == "below":
                    assert status == 0 and hsh == planes_hash(good[c.neighbour].file, planes, (x, y, bw, bh)), (c.name, x, y, bw, bh)
                else:
                    assert status == pc.INVALID_IDAT and hsh == 0, (c.name, x, y, bw, bh, where)
                seen.add(("filter", where))
    # palette indices: (y, x) of the places of unfilter_cases._refusals
    for place, py, px in (("first", 0, 0), ("row63", 63, 37), ("row64", 64, 5), ("row129", 129, 33), ("last", 129, w - 1)):
        c = bad[f"palette10_index_{place}"]
        files = Files(d, f"bad_{c.name}", [c.file])
        boxes = [(px, py, 1, 1, "inside"), (0, 0, w, 130, "inside"), (max(0, px - 1), max(0, py - 1), min(3, w - max(0, px - 1)), min(3, 130 - max(0, py - 1)), "inside")]
        if py:
            boxes += [(0, 0, w, py, "below"), (px, py - 1, 1, 1, "below")]
        if px:
            boxes += [(0, 0, px, 130, "right"), (px - 1, py, 1, 1, "right")]
        if py < 129:
            boxes += [(0, py + 1, w, 129 - py, "above"), (px, py + 1, 1, 1, "above")]
        if px < w - 1:
            boxes += [(px + 1, 0, w - 1 - px, 130, "left"), (px + 1, py, 1, 1, "left")]
        for x, y, bw, bh, where in boxes:
            for planes in (3, 4):
                status, hsh, guard = run_box(exe, files.paths, planes, (x, y, bw, bh))[0]
                assert guard == 1
                if where == "inside":
                    assert status == pc.INVALID_IDAT and hsh == 0, (c.name, x, y, bw, bh)
                else:
                    assert status == 0 and hsh == planes_hash(good[c.neighbour].file, planes, (x, y, bw, bh)), (c.name, x, y, bw, bh, where)
                seen.add(("palette", where))
    assert seen == {("filter", "inside"), ("filter", "below"), ("filter", "above"), ("palette", "inside"), ("palette", "below"), ("palette", "right"),
                    ("palette", "above"), ("palette", "left")}


def test_a_short_stream_is_refused_whatever_the_box(twins):
    """the stream is inflated and checked to its end: a file whose stream yields fewer than h rows is INVALID_IDAT even for a box
    whose rows are all there"""
    plain, _, d = twins
    c = square_cases()[2]
    import zlib
    short = pc.png(c.w, c.h, c.color, zlib.compress(c.scan[:100 * (1 + 3 * c.w)], 1))
    files = Files(d, "short_stream", [short, c.file])
    got = run_box(plain, files.paths, 3, (0, 0, 16, 16))
    assert got[0] == (pc.INVALID_IDAT, 0, 1) and got[1][0] == 0
