"""CPU tests of fpng_amd.dest_layout(): a uint8 (h, w, c) tensor view -> (d_pixels, row_pitch, FPNG_AMD_SRC_* format) of the pixels
a decode writes in place (Encoder.decode_device_ex / decode_batch_ex), from strides and data_ptr() alone; and of the descriptor
make_decode_batch_ex() builds from it.  No GPU."""
import ctypes

import pytest
import torch

import fpng_amd
from fpng_amd import SRC_FORMATS, _lib

F = {k: v[0] for k, v in SRC_FORMATS.items()}


def test_packed_views_every_order():
    rgb = torch.zeros((5, 7, 3), dtype=torch.uint8)
    for order in ("rgb", "bgr"):
        assert fpng_amd.dest_layout(rgb, order) == (rgb.data_ptr(), 21, F[order.upper()])
    rgba = torch.zeros((5, 7, 4), dtype=torch.uint8)
    for order in ("rgba", "bgra", "argb", "abgr", "rgbx", "bgrx", "xrgb", "xbgr"):
        assert fpng_amd.dest_layout(rgba, order) == (rgba.data_ptr(), 28, F[order.upper()])
        assert fpng_amd.dest_layout(rgba, order.upper())[2] == F[order.upper()]
    assert fpng_amd.dest_layout(rgba)[2] == F["RGBA"]  # (alpha last)
    assert fpng_amd.dest_layout(rgba, "bgr")[2] == F["BGRA"]


def test_crop_keeps_the_parent_pitch():
    big = torch.zeros((100, 200, 4), dtype=torch.uint8)
    crop = big[10:30, 17:60]
    assert fpng_amd.dest_layout(crop, "bgra") == (big.data_ptr() + (10 * 200 + 17) * 4, 800, F["BGRA"])
    big3 = torch.zeros((40, 33, 3), dtype=torch.uint8)
    crop3 = big3[3:9, 5:6]  # one pixel wide, odd start byte
    assert fpng_amd.dest_layout(crop3, "bgr") == (big3.data_ptr() + (3 * 33 + 5) * 3, 99, F["BGR"])


def test_padded_pitch():
    b = torch.zeros((8, 10 * 4 + 256), dtype=torch.uint8)
    v = b[:, :40].view(8, 10, 4)
    assert fpng_amd.dest_layout(v, "bgrx") == (b.data_ptr(), 296, F["BGRX"])
    b3 = torch.zeros((8, 31), dtype=torch.uint8)
    v3 = b3[:, :30].view(8, 10, 3)
    assert fpng_amd.dest_layout(v3) == (b3.data_ptr(), 31, F["RGB"])


def test_bottom_up():
    rgba = torch.zeros((6, 9, 4), dtype=torch.uint8)
    assert fpng_amd.dest_layout(rgba, "rgba", bottom_up=True) == (rgba.data_ptr() + 5 * 36, -36, F["RGBA"])
    rgb = torch.zeros((4, 5, 3), dtype=torch.uint8)
    assert fpng_amd.dest_layout(rgb, "bgr", bottom_up=True) == (rgb.data_ptr() + 3 * 15, -15, F["BGR"])
    crop = torch.zeros((10, 20, 4), dtype=torch.uint8)[2:6, 4:9]
    assert fpng_amd.dest_layout(crop, "xbgr", bottom_up=True) == (crop.data_ptr() + 3 * 80, -80, F["XBGR"])
    one = torch.zeros((1, 5, 3), dtype=torch.uint8)
    assert fpng_amd.dest_layout(one, bottom_up=True) == (one.data_ptr(), 0, F["RGB"])  # one row: no pitch


def test_dest_bytes():
    for name, (v, sb, _c) in SRC_FORMATS.items():
        assert fpng_amd.dest_bytes(v) == sb == (3 if name in ("RGB", "BGR") else 4)


def test_rejections():
    rgb = torch.zeros((4, 5, 3), dtype=torch.uint8)
    rgba = torch.zeros((4, 5, 4), dtype=torch.uint8)
    with pytest.raises(ValueError):  # three channels of 4-byte pixels: the decoder would write the fourth byte
        fpng_amd.dest_layout(rgba[..., :3])
    with pytest.raises(ValueError):
        fpng_amd.dest_layout(rgba[..., 1:], "bgr")
    with pytest.raises(ValueError):  # ... also one pixel wide
        fpng_amd.dest_layout(rgba[:, :1, :3])
    for view, order in ((rgb, "rgba"), (rgb, "rgbx"), (rgb, "xrg"), (rgba, "rgbb"), (rgba, "rgxa"), (rgba, "bgrxa")):
        with pytest.raises(ValueError):  # an order that does not name the view's channels
            fpng_amd.dest_layout(view, order)
    with pytest.raises(ValueError):  # overlapping rows
        fpng_amd.dest_layout(torch.zeros(64, dtype=torch.uint8).as_strided((4, 5, 3), (6, 3, 1)))
    with pytest.raises(ValueError):  # stride 0: every row is the same memory
        fpng_amd.dest_layout(torch.zeros((1, 5, 4), dtype=torch.uint8).expand(4, 5, 4))
    with pytest.raises(ValueError):  # stride 0 along the row
        fpng_amd.dest_layout(torch.zeros((4, 1, 3), dtype=torch.uint8).expand(4, 5, 3))
    with pytest.raises(ValueError):  # channels not adjacent
        fpng_amd.dest_layout(torch.zeros((4, 3, 5), dtype=torch.uint8).permute(0, 2, 1))
    for dt in (torch.float32, torch.int8, torch.int16):
        with pytest.raises(ValueError):  # other dtypes
            fpng_amd.dest_layout(torch.zeros((4, 5, 3), dtype=dt))
    with pytest.raises(ValueError):
        fpng_amd.dest_layout(torch.zeros((4, 5, 2), dtype=torch.uint8))
    with pytest.raises(ValueError):
        fpng_amd.dest_layout(torch.zeros((4, 5), dtype=torch.uint8))


def test_png_ex_record():
    # fpng_amd_png_ex: 40 bytes, no padding (include/fpng_amd.h)
    assert ctypes.sizeof(_lib.PngExIn) == 40
    assert [getattr(_lib.PngExIn, f).offset for f in ("data", "size", "format", "d_pixels", "row_pitch", "pixels_cap")] == [0, 8, 12, 16, 24, 32]


def test_entry_points_are_exported():
    lib = _lib.load()
    for name in ("fpng_amd_decode_batch_ex", "fpng_amd_decode_batch_device_ex"):
        assert getattr(lib, name) is not None
