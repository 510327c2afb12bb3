"""No-GPU tests of the crop decode interface (fpng_amd_decode_batch(_device)_planar_crop, fpng_amd_decode_crop_tiles): the exported
symbols and the fpng_amd_crop record, the tiles a crop needs against a Python restatement of the rule, and the descriptor
make_decode_batch_crop builds from CPU tensor views (it only reads strides and data_ptr())."""
import ctypes as C

import pytest
import torch

import fpng_amd
from fpng_amd import _lib
from fpng_amd.api import Encoder

ROWS, BLOCK = 48, 256  # fpng_amd/csrc/decode.h: kDecUnfRows, the 256 pixels of a column block
DTYPES = [(torch.uint8, 1), (torch.float32, 4), (torch.float16, 2), (torch.bfloat16, 2)]


def test_entry_points_and_record(built_lib):
    lib = _lib.load()
    for name in ("fpng_amd_decode_batch_planar_crop", "fpng_amd_decode_batch_device_planar_crop", "fpng_amd_decode_crop_tiles"):
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None
    assert lib.fpng_amd_abi_version() == 5  # (new entry points, the same ABI version)
    assert C.sizeof(_lib.Crop) == 16
    assert {n: getattr(_lib.Crop, n).offset for n, _ in _lib.Crop._fields_} == {"x": 0, "y": 4, "w": 8, "h": 12}
    assert _lib.DECODE_CROP_OUTSIDE == fpng_amd.DECODE_CROP_OUTSIDE == 67


def test_null_arguments_are_refused_without_a_device(built_lib):
    lib = _lib.load()
    fmt, crop = _lib.FloatFormat(), (_lib.Crop * 1)()
    crop[0].w = crop[0].h = 1
    for fn in (lib.fpng_amd_decode_batch_planar_crop, lib.fpng_amd_decode_batch_device_planar_crop):
        assert fn(None, None, crop, 1, C.byref(fmt), None) == -1
        assert fn(None, None, crop, 1, None, None) == -1
        assert fn(None, None, None, 1, None, None) == -1
    n = C.c_uint32()
    assert lib.fpng_amd_decode_crop_tiles(10, 10, None, C.byref(n), C.byref(n), C.byref(n)) == -1
    assert lib.fpng_amd_decode_crop_tiles(10, 10, crop, None, C.byref(n), C.byref(n)) == -1


def _tiles(file_w, file_h, crop):
    """the rule, restated: None for an empty crop or one that leaves the image"""
    x, y, w, h = crop
    if w == 0 or h == 0 or x + w > file_w or y + h > file_h:
        return None
    first = x // BLOCK
    return ((y + h + ROWS - 1) // ROWS, first, (x + w - 1) // BLOCK - first + 1)


def _edges(size, marks):
    """crop (start, length) pairs along one axis: every corner, and every span that starts or ends at one of the marks"""
    pts = sorted({0, size} | {m for m in marks if 0 <= m <= size} | {m + 1 for m in marks if m + 1 <= size})
    return [(a, b - a) for a in pts for b in pts if b > a] + [(size - 1, 1), (0, 1)]


def test_crop_tiles_against_the_rule(built_lib):
    checked = 0
    for fw in (1, 255, 256, 257, 600):
        for fh in (1, 47, 48, 49, 130):
            for x, w in _edges(fw, (255, 256, 257, 511, 512)):
                for y, h in _edges(fh, (47, 48, 49, 95, 96)):
                    want = _tiles(fw, fh, (x, y, w, h))
                    assert want is not None
                    assert fpng_amd.crop_tiles(fw, fh, (x, y, w, h)) == want, (fw, fh, x, y, w, h)
                    checked += 1
            for bad in ((0, 0, 0, 1), (0, 0, 1, 0), (fw, 0, 1, 1), (0, fh, 1, 1), (0, 0, fw + 1, 1), (0, 0, 1, fh + 1), (1, 0, fw, 1), (0, 1, 1, fh),
                        (0xFFFFFFFF, 0, 2, 1), (0, 0xFFFFFFFF, 1, 2)):
                assert _tiles(fw, fh, bad) is None
                with pytest.raises(fpng_amd.FpngAmdError) as e:
                    fpng_amd.crop_tiles(fw, fh, bad)
                assert e.value.code == -1, bad
    assert checked > 1000
    assert fpng_amd.crop_tiles(600, 130, (256, 0, 256, 1)) == (1, 1, 1)
    assert fpng_amd.crop_tiles(600, 130, (255, 0, 2, 1)) == (1, 0, 2)
    assert fpng_amd.crop_tiles(600, 130, (0, 40, 1, 8))[0] == 1   # y + h = 48
    assert fpng_amd.crop_tiles(600, 130, (0, 40, 1, 9))[0] == 2   # y + h = 49
    assert fpng_amd.crop_tiles(600, 130, (0, 0, 600, 130)) == (3, 0, 3)
    assert fpng_amd.crop_tiles(600, 130, (599, 129, 1, 1)) == (3, 2, 1)


@pytest.mark.parametrize("dtype,e", DTYPES)
def test_descriptor_from_views(built_lib, dtype, e):
    """byte pitches and pixels_cap of crop-sized views of a larger canvas; the crops as given; fmt only for float destinations"""
    canvas = torch.zeros(4, 3, 300, 400, dtype=dtype)
    crops = [(5, 7, 9, 11), (250, 40, 13, 20), (0, 0, 224, 224), (61, 0, 7, 1)]
    outs = [canvas[i, :, 10:10 + h, 20:20 + w] for i, (_, _, w, h) in enumerate(crops)]
    pngs = [b"\x89PNG" + bytes(60)] * 4  # (host files: only their address and size are recorded)
    db = Encoder.make_decode_batch_crop(pngs, crops, outs, bottom_up=[False, True, False, False])
    assert isinstance(db, fpng_amd.DecodeBatchCrop) and not db.device_data
    assert (db.fmt is None) == (dtype == torch.uint8)
    if db.fmt is not None:
        assert db.fmt.dtype == fpng_amd.FLOAT_DTYPES[dtype] and db.fmt.reserved == 0
    for i, (x, y, w, h) in enumerate(crops):
        r, c = db.arr[i], db.crops[i]
        assert (c.x, c.y, c.w, c.h) == (x, y, w, h)
        rp = 400 * e if h > 1 else 0
        first = outs[i].data_ptr()
        assert r.num_chans == 3 and r.size == 64
        assert r.plane_pitch == 300 * 400 * e
        assert (r.d_pixels, r.row_pitch) == ((first + (h - 1) * rp, -rp) if i == 1 else (first, rp))
        assert r.pixels_cap == 2 * 300 * 400 * e + (h - 1) * abs(rp) + w * e
    with pytest.raises(ValueError):  # a destination that is not the crop's size
        Encoder.make_decode_batch_crop(pngs[:1], [(0, 0, 9, 11)], [canvas[0, :, :11, :10]])
    with pytest.raises(ValueError):
        Encoder.make_decode_batch_crop(pngs[:1], [(0, 0, 9, 11)], [canvas[0, :, :9, :11]])
    other = torch.zeros(3, 11, 9, dtype=torch.float16 if dtype != torch.float16 else torch.float32)
    with pytest.raises(ValueError):  # mixed dtypes
        Encoder.make_decode_batch_crop(pngs[:2], [(0, 0, 9, 11)] * 2, [canvas[0, :, :11, :9], other])
    with pytest.raises(ValueError):  # one crop per file
        Encoder.make_decode_batch_crop(pngs[:2], [(0, 0, 9, 11)], [canvas[0, :, :11, :9], canvas[1, :, :11, :9]])
    with pytest.raises(ValueError):
        Encoder.make_decode_batch_crop(pngs[:1], [(-1, 0, 9, 11)], [canvas[0, :, :11, :9]])
    if dtype == torch.uint8:
        for kw in ({"mean": (0.5,) * 3, "std": (0.5,) * 3}, {"scale": [1.0]}, {"bias": [0.0]}):
            with pytest.raises(ValueError):  # float arguments with uint8 destinations
                Encoder.make_decode_batch_crop(pngs[:1], [(0, 0, 9, 11)], [canvas[0, :, :11, :9]], **kw)
    else:
        db = Encoder.make_decode_batch_crop(pngs[:1], [(0, 0, 9, 11)], [canvas[0, :, :11, :9]], mean=(0.5,) * 3, std=(0.25,) * 3)
        assert db.fmt.scale[0] == pytest.approx(1 / (255 * 0.25)) and db.fmt.bias[2] == -2.0 and db.fmt.bias[3] == 0.0
