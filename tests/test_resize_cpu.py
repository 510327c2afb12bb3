"""No-GPU tests of the resize decode interface (fpng_amd_decode_batch(_device)_planar_resize, fpng_amd_resize_weights): the exported
symbols and the fpng_amd_resize record, the refusals that need no device, the library's weights against the Python restatement of the
rule (resize_model.py), that restatement against Pillow itself, and the descriptor make_decode_batch_resize builds from CPU tensor
views (it only reads strides and data_ptr())."""
import ctypes as C

import numpy as np
import pytest
import torch

import fpng_amd
from fpng_amd import _lib
from fpng_amd.api import Encoder

import resize_model as RM

DTYPES = [(torch.uint8, 1), (torch.float32, 4), (torch.float16, 2), (torch.bfloat16, 2)]
NAMES = ("fpng_amd_decode_batch_planar_resize", "fpng_amd_decode_batch_device_planar_resize", "fpng_amd_resize_weights")


def test_entry_points_and_record(built_lib):
    lib = _lib.load()
    for name in NAMES:
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None
    assert lib.fpng_amd_abi_version() == 5  # (new entry points, the same ABI version)
    assert C.sizeof(_lib.Resize) == 16
    assert {n: getattr(_lib.Resize, n).offset for n, _ in _lib.Resize._fields_} == {"out_w": 0, "out_h": 4, "flags": 8, "reserved": 12}
    assert _lib.RESIZE_MIRROR == fpng_amd.RESIZE_MIRROR == 1


def _records(crop, size):
    c, s = (_lib.Crop * 1)(), (_lib.Resize * 1)()
    c[0].x, c[0].y, c[0].w, c[0].h = crop
    s[0].out_w, s[0].out_h, s[0].flags, s[0].reserved = size
    return c, s


def test_invalid_arguments_are_refused_without_a_device(built_lib):
    """The records are judged before anything else, so with no encoder at all every call returns -1 -- and the message says whether
    a record was the reason: 97 x 64 -> 3 x 2 is refused for its size, 96 x 64 -> 3 x 2 only for the missing encoder."""
    lib = _lib.load()
    fmt = _lib.FloatFormat()
    good_c, good_s = _records((0, 0, 96, 64), (3, 2, 0, 0))

    def why():
        return lib.fpng_amd_last_error().decode()

    for fn in (lib.fpng_amd_decode_batch_planar_resize, lib.fpng_amd_decode_batch_device_planar_resize):
        assert fn(None, None, None, good_s, 1, None, None) == -1 and "null crops" in why()
        assert fn(None, None, good_c, None, 1, C.byref(fmt), None) == -1 and "null sizes" in why()
        for crop, size, word in (((0, 0, 96, 64), (0, 2, 0, 0), "out_w"), ((0, 0, 96, 64), (3, 0, 0, 0), "out_h"), ((0, 0, 96, 64), (3, 2, 0, 1), "reserved"),
                                 ((0, 0, 96, 64), (3, 2, 2, 0), "flags"), ((0, 0, 96, 64), (3, 2, 3, 0), "flags"), ((0, 0, 97, 64), (3, 2, 0, 0), "32"),
                                 ((0, 0, 96, 65), (3, 2, 1, 0), "32"), ((0, 0, 0, 64), (3, 2, 0, 0), "empty crop"), ((0, 0, 96, 0), (3, 2, 0, 0), "empty crop")):
            c, s = _records(crop, size)
            assert fn(None, None, c, s, 1, None, None) == -1 and word in why(), (crop, size, why())
        for flags in (0, 1):  # (exactly 32 x, mirrored or not: no record is at fault -- the batch has no encoder)
            c, s = _records((0, 0, 96, 64), (3, 2, flags, 0))
            assert fn(None, None, c, s, 1, None, None) == -1 and "null/empty batch" in why(), why()
    u, i = C.c_uint32(), C.c_int32()
    assert lib.fpng_amd_resize_weights(4, 2, None, C.byref(u), C.byref(i)) == -1
    assert lib.fpng_amd_resize_weights(4, 2, C.byref(u), None, C.byref(i)) == -1
    assert lib.fpng_amd_resize_weights(4, 2, C.byref(u), C.byref(u), None) == -1
    for bad in ((0, 1), (1, 0), (33, 1), (65, 2)):
        with pytest.raises(fpng_amd.FpngAmdError) as e:
            fpng_amd.resize_weights(*bad)
        assert e.value.code == -1, bad


GRID = (1, 2, 3, 5, 7, 48, 49, 224, 255, 256, 257, 600)


def _pairs():
    """every pair of GRID inside the 32 x limit (the others are refused: test below), the named ones, 200 seeded ones"""
    out = [(a, b) for a in GRID for b in GRID if a <= RM.MAX_SCALE * b]
    out += [(1080, 224), (1920, 224), (96, 3), (64, 2)]
    rng = np.random.default_rng(2024)
    seeded = 0
    while seeded < 200:
        a, b = int(rng.integers(1, 3000)), int(rng.integers(1, 700))
        if a <= RM.MAX_SCALE * b:
            out.append((a, b))
            seeded += 1
    return out


def test_weights_against_the_rule(built_lib):
    """first, count and every weight of fpng_amd_resize_weights equal the restatement's; behind a row's count the weights are 0; a
    row sums to 2^22 within `count` units (each weight is rounded once) and has at most 65 taps"""
    pairs = _pairs()
    assert len(pairs) >= 300 and (224, 7) in pairs and (1, 600) in pairs
    for a, b in ((a, b) for a in GRID for b in GRID if a > RM.MAX_SCALE * b):  # (past the limit: refused, not computed)
        with pytest.raises(fpng_amd.FpngAmdError):
            fpng_amd.resize_weights(a, b)
    for in_size, out_size in pairs:
        first, count, weights = fpng_amd.resize_weights(in_size, out_size)
        mf, mc, mk = RM.axis_weights(in_size, out_size)
        assert first.tolist() == mf and count.tolist() == mc, (in_size, out_size)
        assert weights.shape == (out_size, RM.MAX_TAPS)
        for o in range(out_size):
            n = mc[o]
            assert 1 <= n <= RM.MAX_TAPS and mf[o] + n <= in_size, (in_size, out_size, o)
            assert weights[o, :n].tolist() == mk[o], (in_size, out_size, o)
            assert not weights[o, n:].any() and min(mk[o]) >= 0
            assert abs(sum(mk[o]) - (1 << 22)) <= n, (in_size, out_size, o, sum(mk[o]))
    # in == out: the identity
    first, count, weights = fpng_amd.resize_weights(49, 49)
    assert all(weights[o, int(np.argmax(weights[o]))] == 1 << 22 and weights[o].sum() == 1 << 22 for o in range(49))
    assert [int(first[o] + np.argmax(weights[o])) for o in range(49)] == list(range(49))


NAMED = [((600, 130), (224, 224)), ((1920, 1080), (224, 224)), ((257, 49), (7, 3)), ((8, 8), (224, 224)), ((1, 1), (5, 5)), ((4000, 3), (3, 2))]


def test_the_restatement_is_pillows_resize():
    """resize_model.resize_plane == Image.fromarray(p, "L").resize((ow, oh), Image.BILINEAR), byte for byte: seeded noise and
    two-level (0 / 255) planes at the named sizes and 100 seeded ones"""
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(7)
    cases = list(NAMED) + [((int(rng.integers(1, 90)), int(rng.integers(1, 90))), (int(rng.integers(1, 70)), int(rng.integers(1, 70)))) for _ in range(100)]
    for (w, h), (ow, oh) in cases:
        for kind in ("noise", "levels"):
            p = rng.integers(0, 256, (h, w), dtype=np.uint8)
            if kind == "levels":
                p = ((p & 1) * 255).astype(np.uint8)
            want = np.asarray(Image.fromarray(p, "L").resize((ow, oh), Image.BILINEAR))
            got = RM.resize_plane(p, ow, oh)
            assert got.shape == (oh, ow) and np.array_equal(got, want), ((w, h), (ow, oh), kind, int((got != want).sum()))
    px = rng.integers(0, 256, (3, 33, 47), dtype=np.uint8)
    r = RM.resize_planes(px, 20, 9, mirror=True)
    assert np.array_equal(r[1, :, ::-1], RM.resize_plane(px[1], 20, 9))


@pytest.mark.parametrize("dtype,e", DTYPES)
def test_descriptor_from_views(built_lib, dtype, e):
    """byte pitches and pixels_cap of output-sized views of a larger canvas; the crops as given, the sizes from the views, the
    mirror flag per file; fmt only for float destinations; the refusals"""
    canvas = torch.zeros(4, 3, 300, 400, dtype=dtype)
    crops = [(5, 7, 9, 11), (250, 40, 13, 20), (0, 0, 600, 130), (61, 0, 7, 1)]
    sizes = [(65, 17), (13, 20), (224, 224), (9, 1)]  # (out_w, out_h)
    outs = [canvas[i, :, 10:10 + oh, 20:20 + ow] for i, (ow, oh) in enumerate(sizes)]
    pngs = [b"\x89PNG" + bytes(60)] * 4  # (host files: only their address and size are recorded)
    mirrors = [False, True, True, False]
    db = Encoder.make_decode_batch_resize(pngs, crops, outs, mirror=mirrors, bottom_up=[False, True, False, False])
    assert isinstance(db, fpng_amd.DecodeBatchResize) and not db.device_data
    assert (db.fmt is None) == (dtype == torch.uint8)
    if db.fmt is not None:
        assert db.fmt.dtype == fpng_amd.FLOAT_DTYPES[dtype] and db.fmt.reserved == 0
    for i, ((x, y, w, h), (ow, oh)) in enumerate(zip(crops, sizes)):
        r, c, s = db.arr[i], db.crops[i], db.sizes[i]
        assert (c.x, c.y, c.w, c.h) == (x, y, w, h)
        assert (s.out_w, s.out_h, s.flags, s.reserved) == (ow, oh, 1 if mirrors[i] else 0, 0)
        rp = 400 * e if oh > 1 else 0
        first = outs[i].data_ptr()
        assert r.num_chans == 3 and r.size == 64
        assert r.plane_pitch == 300 * 400 * e
        assert (r.d_pixels, r.row_pitch) == ((first + (oh - 1) * rp, -rp) if i == 1 else (first, rp))
        assert r.pixels_cap == 2 * 300 * 400 * e + (oh - 1) * abs(rp) + ow * e
    for one in (True, False):  # one bool for every file
        db = Encoder.make_decode_batch_resize(pngs, crops, outs, mirror=one)
        assert [s.flags for s in db.sizes] == [1 if one else 0] * 4
    v = canvas[0, :, :11, :9]
    with pytest.raises(ValueError):  # one mirror flag per file
        Encoder.make_decode_batch_resize(pngs[:2], crops[:2], outs[:2], mirror=[True])
    other = torch.zeros(3, 11, 9, dtype=torch.float16 if dtype != torch.float16 else torch.float32)
    with pytest.raises(ValueError):  # mixed dtypes
        Encoder.make_decode_batch_resize(pngs[:2], [(0, 0, 9, 11)] * 2, [v, other])
    with pytest.raises(ValueError):  # one crop per file
        Encoder.make_decode_batch_resize(pngs[:2], [(0, 0, 9, 11)], [v, canvas[1, :, :11, :9]])
    with pytest.raises(ValueError):  # one destination per file
        Encoder.make_decode_batch_resize(pngs[:2], [(0, 0, 9, 11)] * 2, [v])
    with pytest.raises(ValueError):
        Encoder.make_decode_batch_resize(pngs[:1], [(-1, 0, 9, 11)], [v])
    with pytest.raises(ValueError):  # an empty destination
        Encoder.make_decode_batch_resize(pngs[:1], [(0, 0, 9, 11)], [canvas[0, :, :0, :9]])
    if dtype == torch.uint8:
        for kw in ({"mean": (0.5,) * 3, "std": (0.5,) * 3}, {"scale": [1.0]}, {"bias": [0.0]}):
            with pytest.raises(ValueError):  # float arguments with uint8 destinations
                Encoder.make_decode_batch_resize(pngs[:1], [(0, 0, 9, 11)], [v], **kw)
    else:
        db = Encoder.make_decode_batch_resize(pngs[:1], [(0, 0, 90, 110)], [v], mean=(0.5,) * 3, std=(0.25,) * 3)
        assert db.fmt.scale[0] == pytest.approx(1 / (255 * 0.25)) and db.fmt.bias[2] == -2.0 and db.fmt.bias[3] == 0.0
    # list(batch) of an (n, 3, 32, 32) tensor
    batch = torch.zeros(4, 3, 32, 32, dtype=dtype)
    db = Encoder.make_decode_batch_resize(pngs, crops, list(batch))
    assert [(s.out_w, s.out_h) for s in db.sizes] == [(32, 32)] * 4
    assert [r.d_pixels for r in db.arr] == [batch[i].data_ptr() for i in range(4)]
