"""CPU tests of the YUV decode destination (fpng_amd_decode_batch(_device)_yuv_views): the host twin fpng_amd_yuv_surface, which
compiles the text the kernel compiles (csrc/yuv_store.h), against the rule in numpy (yuv_store_model.py) -- every element equal --
the matrix construction, the layouts (nothing outside the elements is written), the round trip through the encode side's rule,
every refusal with its code, and the ABI.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import yuv_store_model as SM
from yuv_model import Layout

INVALID_ARG, TOO_SMALL = -1, -4
SIZES = [(1, 1), (1, 2), (2, 1), (2, 2), (3, 5), (8, 2), (9, 3), (17, 9), (64, 16), (65, 17)]
STANDARDS = ("bt601", "bt709", "bt2020")


@pytest.fixture(scope="module")
def lib(built_lib):
    from fpng_amd import _lib
    return _lib.load()


def test_error_codes_are_the_headers():
    import os
    import re
    from cpu_ref import ROOT
    text = open(os.path.join(ROOT, "include", "fpng_amd.h")).read()
    codes = {k: int(v) for k, v in re.findall(r"#define (FPNG_AMD_ERR_[A-Z_]+) \((-?\d+)\)", text)}
    assert codes["FPNG_AMD_ERR_INVALID_ARG"] == INVALID_ARG and codes["FPNG_AMD_ERR_BUFFER_TOO_SMALL"] == TOO_SMALL


def _format(surface, depth, m):
    from fpng_amd import _lib
    fmt = _lib.YuvStoreFormat()
    fmt.surface, fmt.depth = _lib.YUV_SURFACES[surface], depth
    for c in range(3):
        for k in range(4):
            fmt.m[c][k] = float(m[c][k])
    return fmt


def surface_span(lay):
    """(the lowest plane's top row, the bytes from there to the last element of the highest plane), by the planes' own spans"""
    ends = []
    for off, (shape, _) in zip(lay.offsets(), lay.plane_shapes()):
        row = shape[1] * (shape[2] if len(shape) == 3 else 1) * lay.elem
        ends.append(off + (shape[0] - 1) * lay.pitch + row)
    return min(lay.offsets()), max(ends) - min(lay.offsets())


def _dest(lay, base, cap=None):
    from fpng_amd import _lib
    rec = _lib.YuvDest()
    rec.d_luma, rec.row_pitch, rec.chroma_offset = base + lay.luma, lay.pitch, lay.chroma_offset
    rec.surface_cap = surface_span(lay)[1] if cap is None else cap
    return rec


def _twin(lib, rgb, lay, depth, m, buf):
    rgb = np.ascontiguousarray(rgb)
    fmt, rec = _format(lay.surface, depth, m), _dest(lay, buf.ctypes.data)
    return lib.fpng_amd_yuv_surface(rgb.ctypes.data, rgb.shape[1], rgb.shape[0], C.byref(fmt), C.byref(rec))


def _expected(buf, lay, rgb, depth, m):
    exp = buf.copy()
    SM.write(SM.surface(rgb, lay.surface, depth, m), lay.numpy_views(exp))
    return exp


@pytest.mark.parametrize("surface,depth", SM.CASES)
def test_twin_equals_the_model(lib, surface, depth):
    """every element, every size: 1 x 1 up to one past a strip and a tile in both directions; random bytes plus the corner colours"""
    import fpng_amd
    rng = np.random.default_rng(7)
    for n, (w, h) in enumerate(SIZES):
        rgb = SM.content(rng, w, h)
        m = SM.matrix(STANDARDS[n % 3], bool(n & 1))
        got = fpng_amd.yuv_surface(rgb, surface, depth, matrix=m)
        want = SM.surface(rgb, surface, depth, m)
        assert len(got) == len(want)
        for k, (a, b) in enumerate(zip(got, want)):
            assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b), (w, h, k)
    # the corner patch whole: block sums 0 .. 1020 with means ending in .25, .5, .75 under both ranges
    patch = SM.corner_patch()
    for full in (False, True):
        m = SM.matrix("bt709", full)
        for a, b in zip(fpng_amd.yuv_surface(patch, surface, depth, matrix=m), SM.surface(patch, surface, depth, m)):
            assert np.array_equal(a, b)


def test_block_means_cover_every_quarter():
    for k in range(3):
        s = SM.block_sums(SM.corner_patch()[..., k])
        assert {int(v) % 4 for v in s.ravel()} == {0, 1, 2, 3}, k
    # an odd edge: the existing pixels count twice
    p = np.array([[1, 2, 3]], dtype=np.uint8)
    assert SM.block_sums(p).tolist() == [[6, 12]]


def test_matrix_is_the_models_bit_for_bit(lib):
    import fpng_amd
    for st in STANDARDS:
        for full in (False, True):
            got = fpng_amd.yuv_matrix_from_rgb(st, full)
            assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), SM.matrix(st, full).view(np.uint32)), (st, full)
    m = (C.c_float * 12)()
    assert lib.fpng_amd_yuv_matrix_from_rgb(3, 0, m) == INVALID_ARG
    assert lib.fpng_amd_yuv_matrix_from_rgb(0, 0, None) == INVALID_ARG


@pytest.mark.parametrize("surface,depth", SM.CASES)
def test_greys(lib, surface, depth):
    """every grey (k, k, k): chroma exactly 128 << (d - 8) in every standard and range; in full range luma exactly k << (d - 8)"""
    import fpng_amd
    grey = np.repeat(np.arange(256, dtype=np.uint8).reshape(16, 16, 1), 3, axis=2)
    shift = 16 - depth if depth > 8 else 0
    for st in STANDARDS:
        for full in (False, True):
            planes = fpng_amd.yuv_surface(grey, surface, depth, standard=st, full_range=full)
            for p in planes[1:]:
                assert np.all(p.astype(np.int64) == (128 << (depth - 8)) << shift), (st, full)
            if full:
                assert np.array_equal(planes[0].astype(np.int64), (grey[..., 0].astype(np.int64) << (depth - 8)) << shift), st


LAYOUTS = [dict(pitch_pad=0), dict(pitch_pad=6), dict(place="far"), dict(place="front", pitch_pad=2), dict(start="odd"), dict(start="odd", place="front", pitch_pad=4)]


def layout_of(surface, w, h, kw):
    """one of LAYOUTS for a surface: start "odd" = 8-bit planes at an odd byte, 16-bit planes at 2 mod 4"""
    kw = dict(kw)
    if kw.get("start") == "odd":
        kw["start"] = 1 if SM.elem_bytes(surface) == 1 else 2
    kw["pitch_pad"] = kw.get("pitch_pad", 0) * SM.elem_bytes(surface) if SM.elem_bytes(surface) == 2 else kw.get("pitch_pad", 0)
    return Layout(surface, w, h, **kw)


@pytest.mark.parametrize("surface,depth", SM.CASES)
def test_layouts_write_the_elements_and_nothing_else(lib, surface, depth):
    """padded pitch, the chroma far away, the chroma in front of the luma, 8-bit planes at an odd byte, 16-bit planes at 2 mod 4: the
    whole buffer, prefilled with random bytes, equals the buffer with the model's elements written into the planes"""
    rng = np.random.default_rng(11)
    m = SM.matrix("bt601", False)
    for kw in LAYOUTS:
        for (w, h) in ((17, 9), (8, 2), (1, 1)):
            lay = layout_of(surface, w, h, kw)
            rgb = SM.content(rng, w, h)
            buf = np.empty(lay.total + 8, dtype=np.uint8)
            buf = buf[(-buf.ctypes.data) % 4:][:lay.total]  # (the base on a dword: `start` alone decides the planes' alignment)
            buf[:] = rng.integers(0, 256, lay.total, dtype=np.uint8)
            exp = _expected(buf, lay, rgb, depth, m)
            assert _twin(lib, rgb, lay, depth, m, buf) == 0, (kw, w, h)
            assert np.array_equal(buf, exp), (kw, w, h, int(np.flatnonzero(buf != exp)[0]))


@pytest.mark.parametrize("standard", STANDARDS)
@pytest.mark.parametrize("full", [False, True])
def test_depth_16_round_trips_through_the_encode_sides_rule(lib, standard, full):
    """a 4:4:4 surface of depth 16, converted back by fpng_amd_yuv_pixels under fpng_amd_yuv_matrix's matrix of the same standard and
    range, returns the R, G, B bytes: random pixels and the corner grid"""
    import fpng_amd
    rng = np.random.default_rng(3)
    rgb = np.concatenate([rng.integers(0, 256, (160, 18, 3), dtype=np.uint8), SM.corner_patch()])
    planes = fpng_amd.yuv_surface(rgb, "yuv444_16", 16, standard=standard, full_range=full)
    back = fpng_amd.yuv_pixels([planes], "yuv444_16", standard=standard, full_range=full)
    assert np.array_equal(back, rgb)


def test_refusals(lib):
    """every refusal of the record and the format, each with its code (the twin judges them as the call does)"""
    from fpng_amd import _lib
    rng = np.random.default_rng(5)
    m = SM.matrix("bt709", False)
    w, h = 9, 5
    rgb = SM.content(rng, w, h)

    def run(surface="nv12", depth=0, mat=m, fmt_null=False, dest_null=False, rgb_=rgb, size=(w, h), **words):
        lay = Layout(surface, w, h, pitch_pad=2)
        buf = np.zeros(lay.total + 64, dtype=np.uint8)
        rec = _dest(lay, buf.ctypes.data)
        for k, v in words.items():
            setattr(rec, k, v(rec, lay) if callable(v) else v)
        fmt = _format(surface, depth, mat)
        return lib.fpng_amd_yuv_surface(rgb_.ctypes.data if rgb_ is not None else None, size[0], size[1], None if fmt_null else C.byref(fmt), None if dest_null else C.byref(rec))

    assert run() == 0
    assert run(fmt_null=True) == INVALID_ARG and run(dest_null=True) == INVALID_ARG
    assert run(rgb_=None) == INVALID_ARG and run(size=(0, 5)) == INVALID_ARG and run(size=(9, 0)) == INVALID_ARG
    # an unknown surface
    fmt = _format("nv12", 0, m)
    fmt.surface = 4
    lay = Layout("nv12", w, h)
    buf = np.zeros(lay.total, dtype=np.uint8)
    rec = _dest(lay, buf.ctypes.data)
    assert lib.fpng_amd_yuv_surface(rgb.ctypes.data, w, h, C.byref(fmt), C.byref(rec)) == INVALID_ARG
    # a depth the surface does not have
    for surface, bad in (("nv12", 10), ("nv12", 16), ("yuv444", 12), ("p016", 8), ("p016", 11), ("yuv444_16", 14), ("yuv444_16", 17)):
        assert run(surface, bad) == INVALID_ARG, (surface, bad)
    for surface, good in (("nv12", 8), ("yuv444", 0), ("p016", 0), ("p016", 10), ("yuv444_16", 12), ("yuv444_16", 16)):
        assert run(surface, good) == 0, (surface, good)
    # a bad matrix entry
    for bad in (np.nan, np.inf, -np.inf, 65537.0, -70000.0):
        mm = m.copy()
        mm[1, 2] = bad
        assert run(mat=mm) == INVALID_ARG, bad
    mm = m.copy()
    mm[2, 3] = 65536.0
    assert run(mat=mm) == 0
    # the record
    assert run(reserved=1) == INVALID_ARG
    assert run(row_pitch=-16) == INVALID_ARG
    assert run(row_pitch=w - 1) == INVALID_ARG                       # below w elements
    assert run(row_pitch=w) == INVALID_ARG                           # 4:2:0: below 2 ceil(w / 2) = 10 elements
    assert run("yuv444", row_pitch=w, chroma_offset=h * w) == 0      # (4:4:4: w elements are a row)
    assert run("p016", row_pitch=2 * w) == INVALID_ARG               # 16-bit: the same in bytes
    assert run("p016", row_pitch=21) == INVALID_ARG                  # 16-bit: words not multiples of 2
    assert run("p016", chroma_offset=lambda r, lay: r.chroma_offset + 1) == INVALID_ARG
    assert run("yuv444_16", d_luma=lambda r, lay: r.d_luma + 1) == INVALID_ARG
    assert run("nv12", d_luma=lambda r, lay: r.d_luma + 1, surface_cap=lambda r, lay: r.surface_cap) == 0  # (8-bit planes start anywhere)
    # overlapping planes: |chroma_offset| below the luma plane's span
    span = lambda r: (h - 1) * r.row_pitch + w
    assert run(chroma_offset=lambda r, lay: span(r) - 1) == INVALID_ARG
    assert run(chroma_offset=lambda r, lay: -(span(r) - 1)) == INVALID_ARG
    assert run("yuv444", chroma_offset=lambda r, lay: span(r) - 1) == INVALID_ARG
    assert run(chroma_offset=lambda r, lay: span(r), surface_cap=1 << 20) == 0
    # room
    assert run(d_luma=None) == TOO_SMALL
    assert run(surface_cap=lambda r, lay: r.surface_cap - 1) == TOO_SMALL
    assert run("yuv444_16", surface_cap=lambda r, lay: r.surface_cap - 1) == TOO_SMALL
    front = Layout("nv12", w, h, place="front")
    buf = np.zeros(front.total, dtype=np.uint8)
    rec = _dest(front, buf.ctypes.data)
    fmt = _format("nv12", 0, m)
    assert lib.fpng_amd_yuv_surface(rgb.ctypes.data, w, h, C.byref(fmt), C.byref(rec)) == 0
    rec.surface_cap -= 1
    assert lib.fpng_amd_yuv_surface(rgb.ctypes.data, w, h, C.byref(fmt), C.byref(rec)) == TOO_SMALL


def test_the_views_call_refuses_before_it_looks_at_the_encoder(lib):
    """fpng_amd_decode_batch(_device)_yuv_views: a null fmt or dests, a bad format, a bad record and num_chans != 3 are refused with
    INVALID_ARG with no encoder at hand -- nothing is launched"""
    from fpng_amd import _lib
    m = SM.matrix("bt709", False)
    files = (_lib.PngPlanarIn * 1)()
    png = (C.c_uint8 * 64)()
    files[0].data, files[0].size, files[0].num_chans = C.addressof(png), 64, 3
    counts = (C.c_uint32 * 1)(1)
    crops, views, res = (_lib.Crop * 1)(), (_lib.ResizeView * 1)(), (_lib.DecodeResult * 1)()
    crops[0].w, crops[0].h = 16, 8
    views[0].full_w, views[0].full_h, views[0].w, views[0].h = 16, 8, 16, 8
    lay = Layout("nv12", 16, 8)
    buf = np.zeros(lay.total, dtype=np.uint8)
    dests = (_lib.YuvDest * 1)(_dest(lay, buf.ctypes.data))
    fmt = _format("nv12", 0, m)
    for name in ("fpng_amd_decode_batch_yuv_views", "fpng_amd_decode_batch_device_yuv_views"):
        call = getattr(lib, name)
        assert call(None, files, 1, counts, crops, views, dests, None, res) == INVALID_ARG
        assert call(None, files, 1, counts, crops, views, None, C.byref(fmt), res) == INVALID_ARG
        bad = _format("nv12", 10, m)
        assert call(None, files, 1, counts, crops, views, dests, C.byref(bad), res) == INVALID_ARG
        bad = _format("nv12", 0, m)
        bad.surface = 7
        assert call(None, files, 1, counts, crops, views, dests, C.byref(bad), res) == INVALID_ARG
        dests[0].reserved = 1
        assert call(None, files, 1, counts, crops, views, dests, C.byref(fmt), res) == INVALID_ARG
        assert b"reserved" in lib.fpng_amd_last_error()
        dests[0].reserved = 0
        dests[0].row_pitch = 15
        assert call(None, files, 1, counts, crops, views, dests, C.byref(fmt), res) == INVALID_ARG
        dests[0].row_pitch = -16
        assert call(None, files, 1, counts, crops, views, dests, C.byref(fmt), res) == INVALID_ARG
        dests[0].row_pitch = lay.pitch
        dests[0].chroma_offset = 7 * 16 + 15
        assert call(None, files, 1, counts, crops, views, dests, C.byref(fmt), res) == INVALID_ARG
        assert b"overlap" in lib.fpng_amd_last_error()
        dests[0].chroma_offset = lay.chroma_offset
        files[0].num_chans = 4
        assert call(None, files, 1, counts, crops, views, dests, C.byref(fmt), res) == INVALID_ARG
        assert b"num_chans" in lib.fpng_amd_last_error()
        files[0].num_chans = 3
        files[0].pixels_cap = 1  # (the files' destination fields are NULL / 0, as in the planar views call)
        assert call(None, files, 1, counts, crops, views, dests, C.byref(fmt), res) == INVALID_ARG
        files[0].pixels_cap = 0
        # everything judged: the call now wants its encoder
        assert call(None, files, 1, counts, crops, views, dests, C.byref(fmt), res) == INVALID_ARG
        assert b"null" in lib.fpng_amd_last_error().lower()


def test_abi(lib):
    from fpng_amd import _lib
    assert C.sizeof(_lib.YuvDest) == 40 and C.sizeof(_lib.YuvStoreFormat) == 56
    assert _lib.YuvDest.surface_cap.offset == 24 and _lib.YuvStoreFormat.m.offset == 8
    for name in ("fpng_amd_decode_batch_yuv_views", "fpng_amd_decode_batch_device_yuv_views", "fpng_amd_yuv_matrix_from_rgb", "fpng_amd_yuv_surface"):
        assert hasattr(lib, name), name
    assert lib.fpng_amd_abi_version() == 5


def test_python_layout_words(lib):
    """yuv_surface_planes / yuv_frame_layout / yuv_surface_bytes: a tight surface's words are the header's, its room the planes' span"""
    import fpng_amd
    for surface in SM.SURFACES:
        for (w, h) in ((9, 5), (8, 2), (1, 1)):
            e = SM.elem_bytes(surface)
            planes = fpng_amd.yuv_surface_planes(surface, w, h, lambda n, elem: np.zeros(n, dtype=np.uint8 if elem == 1 else np.uint16))
            _, pitch, co, ww, hh = fpng_amd.yuv_frame_layout(planes, surface)
            lay = Layout(surface, w, h)
            assert (ww, hh) == (w, h) and pitch in (0, lay.pitch) and co == lay.chroma_offset, (surface, w, h)
            assert fpng_amd.yuv_surface_bytes(surface, w, h, pitch, co) == surface_span(lay)[1]
            front = Layout(surface, w, h, place="front", pitch_pad=2 * e)
            assert fpng_amd.yuv_surface_bytes(surface, w, h, front.pitch, front.chroma_offset) == surface_span(front)[1]
