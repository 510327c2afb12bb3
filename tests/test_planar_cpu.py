"""No-GPU tests of the planar (channels-first, CHW) interface: source_layout_planar / dest_layout_planar on tensor views, the two
C records, the three exported entry points, and the descriptors make_batch_planar / make_decode_batch_planar build on CPU tensors
(they only read strides and data_ptr())."""
import ctypes as C

import pytest
import torch

import fpng_amd
from fpng_amd import _lib
from fpng_amd.api import Encoder, dest_layout_planar, source_layout_planar

BOTH = [source_layout_planar, dest_layout_planar]


def _chw(c, h, w):
    return torch.arange(c * h * w, dtype=torch.int64).remainder(251).to(torch.uint8).reshape(c, h, w)


@pytest.mark.parametrize("fn", BOTH)
def test_contiguous_chw(fn):
    for c, h, w in ((3, 5, 7), (4, 5, 7), (3, 1, 9), (4, 9, 1), (3, 1, 1)):
        t = _chw(c, h, w)
        ptr, rp, pp = fn(t)
        assert ptr == t.data_ptr()
        assert rp == (w if h > 1 else 0)  # (one row: no pitch, the C side takes w)
        assert pp == h * w


@pytest.mark.parametrize("fn", BOTH)
def test_image_of_a_batch_and_three_planes_of_four(fn):
    n = torch.zeros(5, 3, 6, 11, dtype=torch.uint8)
    assert fn(n[2]) == (n.data_ptr() + 2 * 3 * 6 * 11, 11, 66)
    rgba = _chw(4, 6, 11)
    assert fn(rgba[:3]) == (rgba.data_ptr(), 11, 66)
    assert fn(rgba[1:]) == (rgba.data_ptr() + 66, 11, 66)


@pytest.mark.parametrize("fn", BOTH)
def test_crop_keeps_the_parents_pitches(fn):
    t = _chw(3, 40, 50)
    v = t[:, 7:19, 3:44]
    assert fn(v) == (t.data_ptr() + 7 * 50 + 3, 50, 2000)
    one_row = t[:, 7:8, 3:44]
    assert fn(one_row) == (t.data_ptr() + 7 * 50 + 3, 0, 2000)


@pytest.mark.parametrize("fn", BOTH)
def test_padded_rows_and_planes(fn):
    buf = torch.zeros(4, 10, 64, dtype=torch.uint8)
    v = buf[:, :, :33]
    assert fn(v) == (buf.data_ptr(), 64, 640)
    far = torch.zeros(3, 3, 10, 33, dtype=torch.uint8)[:, 1]  # planes with other planes between them
    assert fn(far) == (far.data_ptr(), 33, 3 * 10 * 33)


@pytest.mark.parametrize("fn", BOTH)
def test_bottom_up(fn):
    t = _chw(3, 6, 11)
    assert fn(t, bottom_up=True) == (t.data_ptr() + 5 * 11, -11, 66)
    one = _chw(3, 1, 11)
    assert fn(one, bottom_up=True) == (one.data_ptr(), 0, 11)


@pytest.mark.parametrize("fn", BOTH)
def test_reversed_planes(fn):
    t = _chw(3, 6, 11)
    assert fn(t, order="bgr") == (t.data_ptr() + 2 * 66, 11, -66)
    assert fn(t, order="BGR", bottom_up=True) == (t.data_ptr() + 2 * 66 + 5 * 11, -11, -66)
    q = _chw(4, 6, 11)
    assert fn(q, order="abgr") == (q.data_ptr() + 3 * 66, 11, -66)
    assert fn(q, order="rgba") == fn(q, order="rgb") == (q.data_ptr(), 11, 66)
    for bad in ("bgra", "argb", "bgr", "rgbx", "xyz"):
        with pytest.raises(ValueError):
            fn(q, order=bad)
    for bad in ("rgba", "abgr", "rbg", ""):
        with pytest.raises(ValueError):
            fn(t, order=bad)


@pytest.mark.parametrize("fn", BOTH)
def test_refusals(fn):
    with pytest.raises(ValueError):
        fn(torch.zeros(3, 4, 5, dtype=torch.float16))
    with pytest.raises(ValueError):
        fn(torch.zeros(3, 4, 5, dtype=torch.int8))
    with pytest.raises(ValueError):
        fn(torch.zeros(2, 3, 4, 5, dtype=torch.uint8))  # rank
    with pytest.raises(ValueError):
        fn(torch.zeros(4, 5, dtype=torch.uint8))
    with pytest.raises(ValueError):
        fn(torch.zeros(2, 4, 5, dtype=torch.uint8))  # 2 planes
    with pytest.raises(ValueError):
        fn(torch.zeros(5, 4, 5, dtype=torch.uint8))
    with pytest.raises(ValueError):
        fn("not a tensor")
    hwc = torch.zeros(6, 11, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="submit_ex"):  # an interleaved view: says so, names the call that takes it
        fn(hwc.permute(2, 0, 1))
    t = _chw(3, 6, 11)
    with pytest.raises(ValueError):
        fn(t[:, :, ::2])  # stride(2) == 2
    with pytest.raises(ValueError):
        fn(t[:1].expand(3, 6, 11))  # plane stride 0
    with pytest.raises(ValueError):
        fn(t[:, :1].expand(3, 6, 11))  # row stride 0
    with pytest.raises(ValueError):
        fn(torch.as_strided(t, (3, 6, 11), (66, 10, 1)))  # rows overlap
    with pytest.raises(ValueError):
        fn(torch.as_strided(t, (3, 6, 11), (65, 11, 1)))  # planes overlap
    with pytest.raises(ValueError):
        fn(torch.as_strided(t, (3, 6, 11), (11, 33, 1)))  # planes interleaved row by row: not one plane after another
    assert fn(torch.as_strided(t, (3, 5, 10), (66, 11, 1)))  # (the same with room: fine)


def test_records():
    assert C.sizeof(_lib.ImagePlanar) == 56
    offs = {n: getattr(_lib.ImagePlanar, n).offset for n, _ in _lib.ImagePlanar._fields_}
    assert offs == {"d_pixels": 0, "row_pitch": 8, "plane_pitch": 16, "w": 24, "h": 28, "num_chans": 32, "reserved": 36, "d_out": 40,
                    "out_cap": 48}
    assert C.sizeof(_lib.PngPlanarIn) == 48
    offs = {n: getattr(_lib.PngPlanarIn, n).offset for n, _ in _lib.PngPlanarIn._fields_}
    assert offs == {"data": 0, "size": 8, "num_chans": 12, "d_pixels": 16, "row_pitch": 24, "plane_pitch": 32, "pixels_cap": 40}


def test_entry_points_exported(built_lib):
    lib = _lib.load()
    for name in ("fpng_amd_encode_submit_planar", "fpng_amd_decode_batch_planar", "fpng_amd_decode_batch_device_planar"):
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None
    assert lib.fpng_amd_abi_version() == 5  # (new entry points, the same ABI version)


def test_null_batches_are_refused_without_a_device(built_lib):
    lib = _lib.load()
    t = C.c_uint64(7)
    assert lib.fpng_amd_encode_submit_planar(None, None, 1, 0, C.byref(t)) == -1
    assert lib.fpng_amd_decode_batch_planar(None, None, 1, None) == -1
    assert lib.fpng_amd_decode_batch_device_planar(None, None, 1, None) == -1


def test_make_batch_planar_on_cpu_tensors():
    n = torch.zeros(2, 4, 6, 11, dtype=torch.uint8)
    outs = [torch.zeros(4096, dtype=torch.uint8) for _ in range(3)]
    images = list(n) + [n[1, :3, 1:5, 2:9]]
    _, _, arr = Encoder.make_batch_planar(images, outs, order=["rgba", "abgr", "bgr"], bottom_up=[False, False, True])
    assert len(arr) == 3
    a = arr[0]
    assert (a.d_pixels, a.row_pitch, a.plane_pitch, a.w, a.h, a.num_chans, a.reserved) == (n.data_ptr(), 11, 66, 11, 6, 4, 0)
    assert (a.d_out, a.out_cap) == (outs[0].data_ptr(), 4096)
    a = arr[1]
    assert (a.d_pixels, a.row_pitch, a.plane_pitch, a.num_chans) == (n[1].data_ptr() + 3 * 66, 11, -66, 4)
    a = arr[2]
    base = n[1].data_ptr() + 1 * 11 + 2
    assert (a.d_pixels, a.row_pitch, a.plane_pitch, a.w, a.h, a.num_chans) == (base + 2 * 66 + 3 * 11, -11, -66, 7, 4, 3)


def test_make_decode_batch_planar_on_cpu_tensors():
    big = torch.zeros(4, 20, 30, dtype=torch.uint8)
    views = [big, big[:3, 2:12, 5:25], big[:3]]
    files = [b"\x89PNG", b"", b"abc"]
    d = Encoder.make_decode_batch_planar(files, views, order=["rgba", "rgb", "bgr"], bottom_up=[False, True, False])
    assert isinstance(d, fpng_amd.DecodeBatchPlanar) and not isinstance(d, fpng_amd.DecodeBatchEx) and not d.device_data
    a = d.arr[0]
    assert (a.size, a.num_chans, a.d_pixels, a.row_pitch, a.plane_pitch, a.pixels_cap) == (4, 4, big.data_ptr(), 30, 600, 3 * 600 + 19 * 30 + 30)
    a = d.arr[1]
    assert a.data is None and a.size == 0
    assert (a.num_chans, a.d_pixels, a.row_pitch, a.plane_pitch) == (3, big.data_ptr() + 2 * 30 + 5 + 9 * 30, -30, 600)
    assert a.pixels_cap == 2 * 600 + 9 * 30 + 20  # the view's own span
    a = d.arr[2]
    assert (a.d_pixels, a.plane_pitch, a.pixels_cap) == (big.data_ptr() + 1200, -600, 2 * 600 + 19 * 30 + 30)
    assert len(d.res) == 3 and list(d.statuses()) == [0, 0, 0]


def test_descriptors_of_the_other_kind_are_refused(built_lib):
    """a planar descriptor handed to the _ex calls, and the other way round: ValueError before any device call"""
    e = Encoder.__new__(Encoder)  # (no device: an encoder object without a handle)
    e.lib, e.h = _lib.load(), None
    planar = Encoder.make_decode_batch_planar([b"x"], [torch.zeros(3, 2, 2, dtype=torch.uint8)])
    for fn in (Encoder.decode_device_ex, Encoder.decode_batch_ex):
        with pytest.raises(ValueError, match="planar"):
            fn(e, planar)
    ex = fpng_amd.DecodeBatchEx([], [], None, None, False, [])
    for fn in (Encoder.decode_device_planar, Encoder.decode_batch_planar):
        with pytest.raises(ValueError, match="_ex"):
            fn(e, ex)
