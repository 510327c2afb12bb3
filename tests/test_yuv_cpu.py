"""CPU tests of fpng_amd_encode_submit_yuv (include/fpng_amd.h, csrc/yuv.h): the host twin fpng_amd_yuv_pixels -- the text the kernels
compile -- against the rule in numpy (yuv_model.py), the matrix helper against its construction, the fp32 rule against the
real-valued conversion, every refusal that happens before the device is touched, the generic entry points' refusal of the internal
kind, the Python descriptors, and the renditions' twin on converted frames.  No GPU."""
import ctypes as C
import math

import numpy as np
import pytest

import yuv_model as ym

INVALID_ARG, BUFFER_TOO_SMALL = -1, -4
SIZES = [(1, 1), (2, 2), (3, 3), (5, 1), (1, 5), (65, 3), (257, 2)]  # (w, h)
STANDARDS = [(s, fr) for s in ("bt601", "bt709", "bt2020") for fr in (False, True)]
NEW_SYMBOLS = ["fpng_amd_encode_submit_yuv", "fpng_amd_yuv_matrix", "fpng_amd_yuv_pixels"]

TIES = np.array([[1, 0, 0, 0.5], [0, 1, 0, 0.5], [0, 0, 1, 0.5]], dtype=np.float32)           # every value k + 0.5
CLAMPS = np.array([[3, 0, 0, -200], [0, -2, 0, 300], [1, 1, -3, 100.25]], dtype=np.float32)   # below 0 and above 255 on every channel


@pytest.fixture(scope="module")
def lib(built_lib):
    from fpng_amd import _lib
    return _lib.load()


def _random_matrix(rng):
    m = rng.normal(0.0, 1.0, (3, 4)).astype(np.float32)
    m[:, 3] = rng.uniform(-128, 128, 3).astype(np.float32)
    return m


# ---- the host twin against the model ----
@pytest.mark.parametrize("surface", ym.SURFACES)
def test_the_twin_is_the_model(built_lib, surface):
    import fpng_amd
    rng = np.random.default_rng(20 + ym.SURFACES.index(surface))
    contents = ["full"] + (["msb10"] if ym.elem_bytes(surface) == 2 else [])
    e = ym.elem_bytes(surface)
    for i, (w, h) in enumerate(SIZES):
        for content in contents:
            place = ("tight", "far", "front")[i % 3]
            lay = ym.Layout(surface, w, h, pitch_pad=(0, 6 * e)[i & 1], place=place, start=(0, e)[(i >> 1) & 1])
            buf, planes = ym.fill_surface(lay, rng, content)
            keep = buf.copy()
            for m in (ym.matrix("bt709", False), ym.matrix("bt601", True), _random_matrix(rng), CLAMPS):
                got = fpng_amd.yuv_pixels([planes], surface=surface, matrix=m)
                assert got.shape == (h, w, 3)
                assert np.array_equal(got, ym.to_rgb(surface, planes, m)), (surface, w, h, content, place)
            assert np.array_equal(buf, keep)  # the source is only read


@pytest.mark.parametrize("surface", ym.SURFACES)
def test_ties_round_to_even_and_both_clamps_are_met(built_lib, surface):
    import fpng_amd
    rng = np.random.default_rng(7)
    lay = ym.Layout(surface, 257, 2)
    buf, planes = ym.fill_surface(lay, rng)
    if lay.elem == 2:
        for p in planes:
            p &= np.uint16(0xFF00)  # whole numbers, so that + 0.5 is a tie
    want = ym.to_rgb(surface, planes, TIES)
    y = ym.elements(planes[0])
    # (the model itself: a tie goes to the even neighbour, 255.5 clamps to 255)
    assert np.array_equal(want[..., 0], np.minimum(2 * np.floor((y + 1) / 2), 255).astype(np.uint8))
    assert np.array_equal(fpng_amd.yuv_pixels([planes], surface=surface, matrix=TIES), want)
    got = fpng_amd.yuv_pixels([planes], surface=surface, matrix=CLAMPS)
    assert np.array_equal(got, ym.to_rgb(surface, planes, CLAMPS))
    assert (got == 0).any(axis=(0, 1)).all() and (got == 255).any(axis=(0, 1)).all()


def test_the_chroma_of_a_block_is_replicated(built_lib):
    import fpng_amd
    rng = np.random.default_rng(3)
    lay = ym.Layout("nv12", 6, 4)
    buf, (y, c) = ym.fill_surface(lay, rng)
    y[...] = 100
    m = np.array([[0, 1, 0, 0], [0, 0, 1, 0], [1, 0, 0, 0]], dtype=np.float32)  # R = Cb, G = Cr, B = Y
    got = fpng_amd.yuv_pixels([(y, c)], surface="nv12", matrix=m)
    for yy in range(4):
        for xx in range(6):
            assert tuple(got[yy, xx]) == (c[yy // 2, xx // 2, 0], c[yy // 2, xx // 2, 1], 100)


# ---- the matrix helper ----
@pytest.mark.parametrize("standard,full_range", STANDARDS)
def test_the_matrix_is_its_construction(built_lib, standard, full_range):
    import fpng_amd
    m = fpng_amd.yuv_matrix(standard, full_range)
    assert m.dtype == np.float32 and m.shape == (3, 4)
    assert np.array_equal(m.view(np.uint32), ym.matrix(standard, full_range).view(np.uint32))
    # greys: (k, 128, 128) -> (k', k', k') on all three channels
    k = np.arange(256, dtype=np.uint8).reshape(1, 256)
    grey = ym.to_rgb("yuv444", (k, np.full_like(k, 128), np.full_like(k, 128)), m)
    if full_range:
        want = k[0].astype(np.int64)
    else:
        want = np.clip(np.floor((k[0].astype(np.float64) - 16) * 255 / 219 + 0.5), 0, 255).astype(np.int64)
        assert want[16] == 0 and want[235] == 255
    for c in range(3):
        assert np.array_equal(grey[0, :, c].astype(np.int64), want), (standard, full_range, c)


def test_bt601_limited_is_the_familiar_matrix(built_lib):
    import fpng_amd
    m = fpng_amd.yuv_matrix("bt601", False)
    f = np.float32
    assert m[0, 0] == m[1, 0] == m[2, 0] == f(1.16438353)
    assert m[0, 2] == f(1.59602678) and m[1, 1] == f(-0.391762286) and m[1, 2] == f(-0.812967658) and m[2, 1] == f(2.01723218)
    assert m[0, 1] == 0 and m[2, 2] == 0
    assert m[0, 3] == f(-222.921570) and m[1, 3] == f(135.575302) and m[2, 3] == f(-276.835846)


def test_the_matrix_helper_refuses(lib):
    m = (C.c_float * 12)()
    assert lib.fpng_amd_yuv_matrix(3, 0, m) == INVALID_ARG
    assert lib.fpng_amd_yuv_matrix(0, 0, None) == INVALID_ARG
    import fpng_amd
    with pytest.raises(ValueError):
        fpng_amd.yuv_matrix("bt470")


# ---- the fp32 rule against the real-valued conversion ----
@pytest.mark.parametrize("standard,full_range", STANDARDS)
def test_the_rule_is_within_one_of_the_real_valued_conversion(built_lib, standard, full_range):
    """200 000 random 8-bit triples: no byte may differ by more than 1 from rint(clip(real-valued t_c)), and at most 0.1 % may
    differ at all (the rule itself measured 1.0e-4 at worst, BT.601 full range: the cap only keeps the test from hiding a failure)."""
    import fpng_amd
    rng = np.random.default_rng(99)
    yuv = rng.integers(0, 256, (3, 1, 200000), dtype=np.uint8)
    got = fpng_amd.yuv_pixels([tuple(yuv)], surface="yuv444", standard=standard, full_range=full_range).astype(np.int64)
    kr, kb = ym.KR_KB[standard]
    kg = 1.0 - kr - kb
    sy, sc, y0 = (1.0, 1.0, 0.0) if full_range else (255.0 / 219.0, 255.0 / 224.0, 16.0)
    y, cb, cr = ((yuv[0, 0].astype(np.float64) - y0) * sy, (yuv[1, 0].astype(np.float64) - 128) * sc, (yuv[2, 0].astype(np.float64) - 128) * sc)
    real = np.stack([y + 2 * (1 - kr) * cr, y - 2 * kb * (1 - kb) / kg * cb - 2 * kr * (1 - kr) / kg * cr, y + 2 * (1 - kb) * cb], axis=-1)
    want = np.rint(np.clip(real, 0, 255)).astype(np.int64)
    diff = np.abs(got[0] - want)
    print(f"{standard} full_range={full_range}: max |diff| {diff.max()}, differing {np.count_nonzero(diff) / diff.size:.2e}")
    assert diff.max() <= 1
    assert np.count_nonzero(diff) <= 0.001 * diff.size


# ---- refusals, against a null encoder: every check comes before the encoder is looked at ----
def _frame(w=8, h=4, pitch=0, chroma=None, luma=0x10000, out=0x200000, cap=1 << 20, reserved=0, elem=1):
    from fpng_amd import _lib
    f = _lib.YuvFrame()
    f.d_luma, f.row_pitch, f.w, f.h, f.reserved, f.d_out, f.out_cap = luma, pitch, w, h, reserved, out, cap
    f.chroma_offset = (pitch or w * elem) * h if chroma is None else chroma
    return f


def _fmt(surface=0, reserved=0, m=None):
    from fpng_amd import _lib
    f = _lib.YuvFormat()
    f.surface, f.reserved = surface, reserved
    m = ym.matrix("bt709", False) if m is None else m
    for c in range(3):
        for k in range(4):
            f.m[c][k] = float(m[c][k])
    return f


def _submit(lib, frames, fmt, renditions=None, pack=None):
    from fpng_amd import _lib
    arr = (_lib.YuvFrame * max(len(frames), 1))(*frames)
    rarr = (_lib.Rendition * len(renditions))(*renditions) if renditions else None
    t = C.c_uint64(77)
    rc = lib.fpng_amd_encode_submit_yuv(None, arr if frames else None, len(frames), C.byref(fmt) if fmt is not None else None, rarr, len(renditions or ()), 0,
                                        C.byref(pack) if pack is not None else None, C.byref(t))
    assert t.value == 77  # no ticket
    return rc, lib.fpng_amd_last_error().decode()


def _with(m, c, k, v):
    m = np.array(m, dtype=np.float32)
    m[c, k] = v
    return m


def test_a_valid_call_gets_as_far_as_the_encoder(lib):
    for surface in range(4):
        e = 2 if surface & 1 else 1
        rc, msg = _submit(lib, [_frame(elem=e), _frame(w=7, h=3, pitch=8 * e, elem=e)], _fmt(surface))
        assert (rc, msg) == (INVALID_ARG, "null encoder"), (surface, msg)
    from fpng_amd import _lib
    pack = _lib.Pack(0x400000, 1 << 24, 16, 0, None, 0)
    assert _submit(lib, [_frame(out=0, cap=0)], _fmt(), pack=pack) == (INVALID_ARG, "null encoder")
    r = _lib.Rendition(0, 0, 1, 1, 5, 3, 4, 4, 0, 0, 0x300000, 1 << 20)
    assert _submit(lib, [_frame(out=0, cap=0)], _fmt(), renditions=[r]) == (INVALID_ARG, "null encoder")


def test_every_refusal(lib):
    from fpng_amd import _lib
    base = ym.matrix("bt709", False)
    cases = [
        ("null fmt", [_frame()], None, "null fmt"),
        ("unknown surface", [_frame()], _fmt(4), "unknown surface"),
        ("fmt reserved", [_frame()], _fmt(reserved=1), "reserved"),
        ("frame reserved", [_frame(reserved=1)], _fmt(), "reserved"),
        ("nan entry", [_frame()], _fmt(m=_with(base, 1, 2, math.nan)), "matrix"),
        ("inf entry", [_frame()], _fmt(m=_with(base, 0, 3, math.inf)), "matrix"),
        ("large entry", [_frame()], _fmt(m=_with(base, 2, 0, -65537.0)), "matrix"),
        ("negative pitch", [_frame(pitch=-8, chroma=64)], _fmt(), "negative"),
        ("pitch below w", [_frame(pitch=7, chroma=64)], _fmt(), "row_pitch < w"),
        ("pitch below w, 16-bit", [_frame(pitch=14, chroma=64, elem=2)], _fmt(1), "row_pitch < w"),
        ("odd width's chroma pair", [_frame(w=7, pitch=7, chroma=64)], _fmt(0), "chroma pair"),
        ("odd width's chroma pair, 16-bit", [_frame(w=7, pitch=14, chroma=128, elem=2)], _fmt(1), "chroma pair"),
        ("16-bit luma at an odd byte", [_frame(luma=0x10001, elem=2)], _fmt(1), "multiples of 2"),
        ("16-bit odd pitch", [_frame(pitch=17, chroma=100, elem=2)], _fmt(3), "multiples of 2"),
        ("16-bit odd chroma offset", [_frame(chroma=65, elem=2)], _fmt(3), "multiples of 2"),
        ("planes overlap", [_frame(chroma=8 * 3 + 7)], _fmt(), "overlap"),
        ("planes overlap, in front", [_frame(chroma=-(8 * 3 + 7))], _fmt(2), "overlap"),
        ("planes overlap, padded pitch", [_frame(pitch=32, chroma=32 * 3 + 7)], _fmt(), "overlap"),
        ("chroma offset 0", [_frame(chroma=0)], _fmt(), "overlap"),
        ("width 0", [_frame(w=0)], _fmt(), "dimensions"),
        ("height 0", [_frame(h=0)], _fmt(), "dimensions"),
        ("width too large", [_frame(w=(1 << 24) + 1, h=1)], _fmt(2), "dimensions"),
        ("null luma", [_frame(luma=0)], _fmt(), "null device pointer"),
        ("no frames", [], _fmt(), "null/empty"),
        ("null d_out", [_frame(out=0)], _fmt(), "null device pointer"),
        ("d_out not aligned", [_frame(out=0x200008)], _fmt(), "16-byte aligned"),
        ("the second frame is judged too", [_frame(), _frame(reserved=2)], _fmt(), "reserved"),
    ]
    for name, frames, fmt, words in cases:
        rc, msg = _submit(lib, frames, fmt)
        assert rc == INVALID_ARG and words in msg, (name, rc, msg)
    rc, msg = _submit(lib, [_frame(cap=100)], _fmt())
    assert rc == BUFFER_TOO_SMALL, msg
    # 8-bit planes may start at any byte, with any pitch
    assert _submit(lib, [_frame(luma=0x10001, pitch=9, chroma=37)], _fmt(0))[1] == "null encoder"
    # packed: the frames name no outputs, and the pack is judged as fpng_amd_encode_submit_packed judges it
    pack = _lib.Pack(0x400000, 1 << 24, 16, 0, None, 0)
    rc, msg = _submit(lib, [_frame()], _fmt(), pack=pack)
    assert rc == INVALID_ARG and "packed submission" in msg
    rc, msg = _submit(lib, [_frame(out=0, cap=0)], _fmt(), pack=_lib.Pack(0x400000, 1 << 24, 24, 0, None, 0))
    assert rc == INVALID_ARG and "align" in msg
    rc, msg = _submit(lib, [_frame(out=0, cap=0)], _fmt(), pack=_lib.Pack(0, 1 << 24, 16, 0, None, 0))
    assert rc == INVALID_ARG and "d_arena" in msg
    # renditions: every rule of fpng_amd_encode_submit_renditions, with three channels
    ok = dict(image=0, filter=0, box_x=0, box_y=0, box_w=0, box_h=0, w=4, h=4, alpha_op=0, reserved=0, d_out=0x300000, out_cap=1 << 20)
    src = [_frame(w=100, out=0, cap=0)]
    for name, change, words, code in [("the frames have outputs", None, "d_out must be NULL", INVALID_ARG),
                                      ("image", dict(image=1), "image >= n_images", INVALID_ARG),
                                      ("filter", dict(filter=6), "filter", INVALID_ARG),
                                      ("alpha_op", dict(alpha_op=1), "alpha_op", INVALID_ARG),
                                      ("box outside", dict(box_x=98, box_w=4, box_h=2), "outside", INVALID_ARG),
                                      ("partly zero box", dict(box_x=1), "empty box", INVALID_ARG),
                                      ("scale", dict(w=1, h=4), "scale", INVALID_ARG),
                                      ("reserved", dict(reserved=1), "reserved", INVALID_ARG),
                                      ("size", dict(w=0), "dimensions", INVALID_ARG),
                                      ("no d_out", dict(d_out=0), "null device pointer", INVALID_ARG),
                                      ("out_cap", dict(out_cap=57), "out_cap", BUFFER_TOO_SMALL)]:
        r = _lib.Rendition(**{**ok, **(change or {})})
        rc, msg = _submit(lib, [_frame()] if change is None else src, _fmt(), renditions=[r])
        assert rc == code and words in msg, (name, rc, msg)
    rc, msg = _submit(lib, src, _fmt(), renditions=[_lib.Rendition(**ok)], pack=pack)
    assert rc == INVALID_ARG and "packed submission" in msg
    # (alpha_op is checked, then ignored: the premultiplied op passes)
    assert _submit(lib, src, _fmt(), renditions=[_lib.Rendition(**{**ok, "alpha_op": 2})])[1] == "null encoder"


def test_the_twin_validates_like_the_submit_call(lib):
    from fpng_amd import _lib
    out = np.zeros(8 * 4 * 3, dtype=np.uint8)
    arr = (_lib.YuvFrame * 1)(_frame(pitch=7, chroma=64))
    assert lib.fpng_amd_yuv_pixels(arr, 1, C.byref(_fmt()), 0, None, out.ctypes.data, out.size) == INVALID_ARG
    arr = (_lib.YuvFrame * 1)(_frame())
    assert lib.fpng_amd_yuv_pixels(arr, 1, None, 0, None, out.ctypes.data, out.size) == INVALID_ARG
    assert lib.fpng_amd_yuv_pixels(arr, 1, C.byref(_fmt()), 1, None, out.ctypes.data, out.size) == INVALID_ARG
    assert lib.fpng_amd_yuv_pixels(arr, 1, C.byref(_fmt()), 0, None, None, out.size) == INVALID_ARG
    assert lib.fpng_amd_yuv_pixels(arr, 1, C.byref(_fmt()), 0, None, out.ctypes.data, out.size - 1) == BUFFER_TOO_SMALL


def test_the_generic_entry_points_do_not_know_the_kind(lib):
    """desc_kind 4 is the library's internal number for YUV frames: the four generic entry points, whose fmt is the float one,
    answer it as any unknown kind"""
    from fpng_amd import _lib
    frames = (_lib.YuvFrame * 1)(_frame(out=0, cap=0))
    r = _lib.Rendition(0, 0, 0, 0, 0, 0, 4, 4, 0, 0, 0x300000, 1 << 20)
    pack = _lib.Pack(0x400000, 1 << 24, 16, 0, None, 0)
    out = np.zeros(64, dtype=np.uint8)
    p = C.cast(frames, C.c_void_p)
    for fmt in (None, C.byref(_lib.FloatFormat())):
        rcs = [lib.fpng_amd_encode_submit_packed(None, 4, p, 1, fmt, 0, C.byref(pack), None),
               lib.fpng_amd_encode_submit_renditions(None, 4, p, 1, fmt, C.byref(r), 1, 0, None, None),
               lib.fpng_amd_renditions_plan(4, p, 1, fmt, C.byref(r), 1, 0, None, None),
               lib.fpng_amd_rendition_pixels(4, p, 1, fmt, C.byref(r), out.ctypes.data, out.size)]
        assert rcs == [INVALID_ARG] * 4
        assert "unknown desc_kind" in lib.fpng_amd_last_error().decode()


def test_the_symbols_and_records(lib):
    from fpng_amd import _lib
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name)
    assert C.sizeof(_lib.YuvFrame) == 56 and C.sizeof(_lib.YuvFormat) == 56
    assert _lib.YuvFrame.w.offset == 24 and _lib.YuvFrame.d_out.offset == 40 and _lib.YuvFormat.m.offset == 8
    assert lib.fpng_amd_abi_version() == 5  # added without changing it


# ---- the Python descriptors ----
@pytest.mark.parametrize("surface", ym.SURFACES)
def test_records_from_tensor_views(built_lib, surface):
    import torch
    import fpng_amd
    rng = np.random.default_rng(5)
    e = ym.elem_bytes(surface)
    for (w, h), pad, place, start in [((8, 4), 0, "tight", 0), ((7, 5), 6 * e, "far", e), ((5, 3), 2 * e, "front", 0), ((1, 1), 0, "far", 0), ((9, 1), 0, "tight", 0),
                                      ((1, 6), 4 * e, "front", e)]:
        lay = ym.Layout(surface, w, h, pitch_pad=pad, place=place, start=start)
        buf, planes = ym.fill_surface(lay, rng)
        t = torch.from_numpy(buf)
        views = lay.torch_views(t)
        ptr, pitch, off, ww, hh = fpng_amd.yuv_frame_layout(views, surface)
        assert (ptr - t.data_ptr(), off, ww, hh) == (lay.luma, lay.chroma_offset, w, h)
        assert pitch == (lay.pitch if h > 1 else 0)  # (a single row has no pitch: 0 = tight)
        m = ym.matrix("bt2020", False)
        assert np.array_equal(fpng_amd.yuv_pixels([views], surface=surface, matrix=m), ym.to_rgb(surface, planes, m))
        assert np.array_equal(fpng_amd.yuv_pixels([planes], surface=surface, matrix=m), ym.to_rgb(surface, planes, m))  # numpy views too


def test_what_the_descriptors_refuse(built_lib):
    import torch
    import fpng_amd
    y, c = torch.zeros((4, 8), dtype=torch.uint8), torch.zeros((2, 4, 2), dtype=torch.uint8)
    wide = torch.zeros((4, 16), dtype=torch.uint8)
    with pytest.raises(ValueError, match="row strides differ"):
        fpng_amd.yuv_frame_layout((wide[:, :8], c), "nv12")
    with pytest.raises(ValueError, match="not tight"):
        fpng_amd.yuv_frame_layout((wide[:, ::2], torch.zeros((2, 4, 2), dtype=torch.uint8)), "nv12")
    with pytest.raises(ValueError, match="not tight"):
        fpng_amd.yuv_frame_layout((y, torch.zeros((2, 4, 4), dtype=torch.uint8)[:, :, :2]), "nv12")  # (pairs four bytes apart)
    buf = torch.zeros(4 * 8 * 4, dtype=torch.uint8)
    p = [buf[k * 32:(k + 1) * 32].view(4, 8) for k in range(4)]
    fpng_amd.yuv_frame_layout((p[0], p[1], p[2]), "yuv444")
    with pytest.raises(ValueError, match="Cr - Cb"):
        fpng_amd.yuv_frame_layout((p[0], p[1], p[3]), "yuv444")
    with pytest.raises(ValueError, match="shaped"):
        fpng_amd.yuv_frame_layout((y, torch.zeros((2, 3, 2), dtype=torch.uint8)), "nv12")
    with pytest.raises(ValueError, match="tensors"):
        fpng_amd.yuv_frame_layout((y, c), "p016")
    with pytest.raises(ValueError, match="tuple of"):
        fpng_amd.yuv_frame_layout((y, c, c), "nv12")
    with pytest.raises(ValueError, match="surface"):
        fpng_amd.yuv_frame_layout((y, c), "nv21")
    with pytest.raises(ValueError, match="3 x 4"):
        fpng_amd.yuv_pixels([(y, c)], matrix=np.eye(3))


# ---- the renditions' twin on converted frames ----
@pytest.mark.parametrize("surface", ["nv12", "p016", "yuv444"])
def test_a_rendition_is_the_rendition_of_the_converted_frame(built_lib, surface):
    import fpng_amd
    rng = np.random.default_rng(11)
    w, h = 37, 23
    lay = ym.Layout(surface, w, h, pitch_pad=2 * ym.elem_bytes(surface), place="far")
    buf, planes = ym.fill_surface(lay, rng)
    m = ym.matrix("bt601", False)
    rgb = np.ascontiguousarray(ym.to_rgb(surface, planes, m))
    boxes = [None, (0, 0, 36, 22), (1, 1, 20, 11), (3, 2, 17, 9), (2, 5, 9, 18), (35, 21, 2, 2), (36, 0, 1, 23)]  # odd and even origins
    for i, box in enumerate(boxes):
        for filt in (("bilinear", "bicubic", "nearest", "box", "hamming", "lanczos")[i % 6], "bilinear"):
            bw, bh = (box[2], box[3]) if box else (w, h)
            r = fpng_amd.rendition(0, (max(bw // 2, 1), max(bh // 2, 1)), box=box, filter=filt)
            got = fpng_amd.yuv_pixels([planes], surface=surface, matrix=m, rendition=r)
            assert np.array_equal(got, fpng_amd.rendition_pixels([rgb], r, kind="image")), (surface, box, filt)
    # a copy: size == box
    r = fpng_amd.rendition(0, (17, 9), box=(3, 2, 17, 9))
    assert np.array_equal(fpng_amd.yuv_pixels([planes], surface=surface, matrix=m, rendition=r), rgb[2:11, 3:20])
    # the record's `image` is not looked at: the frame is chosen by `frame`
    lay2 = ym.Layout(surface, 9, 7)
    _, planes2 = ym.fill_surface(lay2, rng)
    r = fpng_amd.rendition(5, (4, 3), box=(1, 1, 8, 6))
    got = fpng_amd.yuv_pixels([planes, planes2], surface=surface, matrix=m, frame=1, rendition=r)
    r0 = fpng_amd.rendition(0, (4, 3), box=(1, 1, 8, 6))
    assert np.array_equal(got, fpng_amd.rendition_pixels([np.ascontiguousarray(ym.to_rgb(surface, planes2, m))], r0, kind="image"))
