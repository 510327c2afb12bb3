"""CPU tests of fpng_amd.source_layout(): a uint8 (h, w, c) tensor view -> (d_pixels, row_pitch, FPNG_AMD_SRC_* format) for
Encoder.submit_ex, from strides and data_ptr() alone.  No GPU."""
import pytest
import torch

import fpng_amd
from fpng_amd import SRC_FORMATS

F = {k: v[0] for k, v in SRC_FORMATS.items()}


def _buf(h, w, px, pad=0):
    # a 4-byte aligned base (torch's CPU allocations are), rows of w * px + pad bytes
    return torch.zeros((h, w * px + pad), dtype=torch.uint8)


def test_packed_rgb_rgba_and_bgr():
    rgb = torch.zeros((5, 7, 3), dtype=torch.uint8)
    assert fpng_amd.source_layout(rgb) == (rgb.data_ptr(), 21, F["RGB"])
    assert fpng_amd.source_layout(rgb, "bgr") == (rgb.data_ptr(), 21, F["BGR"])
    rgba = torch.zeros((5, 7, 4), dtype=torch.uint8)
    for order in ("rgba", "bgra", "argb", "abgr"):
        assert fpng_amd.source_layout(rgba, order) == (rgba.data_ptr(), 28, F[order.upper()])
    assert fpng_amd.source_layout(rgba, "bgr")[2] == F["BGRA"]  # (alpha last)


def test_crop_keeps_the_parent_pitch():
    big = torch.zeros((100, 200, 4), dtype=torch.uint8)
    crop = big[10:30, 17:60]
    assert fpng_amd.source_layout(crop, "bgra") == (big.data_ptr() + (10 * 200 + 17) * 4, 800, F["BGRA"])
    big3 = torch.zeros((40, 33, 3), dtype=torch.uint8)
    crop3 = big3[3:9, 5:6]  # one pixel wide, odd start byte
    assert fpng_amd.source_layout(crop3) == (big3.data_ptr() + (3 * 33 + 5) * 3, 99, F["RGB"])


def test_rgb_slice_of_four_byte_pixels_is_an_x_format():
    rgba = torch.zeros((6, 9, 4), dtype=torch.uint8)
    assert fpng_amd.source_layout(rgba[..., :3]) == (rgba.data_ptr(), 36, F["RGBX"])
    assert fpng_amd.source_layout(rgba[..., :3], "bgr") == (rgba.data_ptr(), 36, F["BGRX"])
    # [..., 1:] of ARGB / ABGR: the view starts one byte into the pixel, the base moves back to the pixel's first byte
    assert fpng_amd.source_layout(rgba[..., 1:]) == (rgba.data_ptr(), 36, F["XRGB"])
    assert fpng_amd.source_layout(rgba[..., 1:], "bgr") == (rgba.data_ptr(), 36, F["XBGR"])
    crop = rgba[2:5, 3:8, 1:]
    assert fpng_amd.source_layout(crop) == (rgba.data_ptr() + (2 * 9 + 3) * 4, 36, F["XRGB"])


def test_padded_pitch():
    b = _buf(8, 10, 4, pad=256)
    v = b[:, :40].view(8, 10, 4)
    assert fpng_amd.source_layout(v, "bgra") == (b.data_ptr(), 296, F["BGRA"])
    b3 = _buf(8, 10, 3, pad=1)
    v3 = b3[:, :30].view(8, 10, 3)
    assert fpng_amd.source_layout(v3, "bgr") == (b3.data_ptr(), 31, F["BGR"])


def test_bottom_up():
    rgba = torch.zeros((6, 9, 4), dtype=torch.uint8)
    assert fpng_amd.source_layout(rgba, "rgba", bottom_up=True) == (rgba.data_ptr() + 5 * 36, -36, F["RGBA"])
    rgb = torch.zeros((4, 5, 3), dtype=torch.uint8)
    assert fpng_amd.source_layout(rgb, bottom_up=True) == (rgb.data_ptr() + 3 * 15, -15, F["RGB"])
    crop = torch.zeros((10, 20, 4), dtype=torch.uint8)[2:6, 4:9, :3]
    assert fpng_amd.source_layout(crop, "bgr", bottom_up=True) == (crop.data_ptr() + 3 * 80, -80, F["BGRX"])
    one = torch.zeros((1, 5, 3), dtype=torch.uint8)
    assert fpng_amd.source_layout(one, bottom_up=True) == (one.data_ptr(), 0, F["RGB"])  # one row: no pitch


def test_format_channels():
    for name, (v, sb, c) in SRC_FORMATS.items():
        assert fpng_amd.format_channels(v) == c
        assert sb == (3 if name in ("RGB", "BGR") else 4)


def test_rejections():
    rgb = torch.zeros((4, 5, 3), dtype=torch.uint8)
    with pytest.raises(ValueError):  # stride 0: every row is the same memory
        fpng_amd.source_layout(torch.zeros((1, 5, 3), dtype=torch.uint8).expand(4, 5, 3))
    with pytest.raises(ValueError):  # stride 0 along the row
        fpng_amd.source_layout(torch.zeros((4, 1, 3), dtype=torch.uint8).expand(4, 5, 3))
    with pytest.raises(ValueError):  # channels not adjacent: stride(2) != 1
        fpng_amd.source_layout(torch.zeros((4, 3, 5), dtype=torch.uint8).permute(0, 2, 1))
    with pytest.raises(ValueError):  # planar (c, h, w) seen as (h, w, c)
        fpng_amd.source_layout(torch.zeros((3, 4, 5), dtype=torch.uint8).permute(1, 2, 0))
    with pytest.raises(ValueError):  # float
        fpng_amd.source_layout(torch.zeros((4, 5, 3), dtype=torch.float32))
    with pytest.raises(ValueError):  # overlapping rows
        fpng_amd.source_layout(torch.zeros(64, dtype=torch.uint8).as_strided((4, 5, 3), (6, 3, 1)))
    with pytest.raises(ValueError):  # 4 channels cannot sit in 3-byte pixels
        fpng_amd.source_layout(torch.zeros(80, dtype=torch.uint8).as_strided((4, 5, 4), (20, 3, 1)))
    with pytest.raises(ValueError):  # 5-byte pixels
        fpng_amd.source_layout(torch.zeros((4, 5, 5), dtype=torch.uint8)[..., :3])
    with pytest.raises(ValueError):  # an order that does not name the channels
        fpng_amd.source_layout(rgb, "rgba")
    with pytest.raises(ValueError):
        fpng_amd.source_layout(torch.zeros((4, 5, 2), dtype=torch.uint8))
