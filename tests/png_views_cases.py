"""What the GPU tests of the PNG views call share (test_gpu_decode_png_views.py): ordinary files written by Pillow, the views of a
file, the oracle -- decode_device_png of the file, those pixels through the fpng encoder, that file through the existing views calls
-- and one runner for both.  Run as a program it is the groups tests' child: the routing batch in one group, then with
FPNG_AMD_PNG_SCRATCH_LIMIT set in this fresh process to a file per group, and the two compared; with the argument "two" a small
mixed batch in one group and in exactly two, the file that the fpng path leaves UNDECIDED in the second."""
import functools
import io
import os
import struct
import sys
import zlib

import numpy as np

PATTERN = 0x5A


def pillow_file(kind, w, h, seed):
    """an ordinary PNG of one colour type, written by Pillow; smooth with some noise, so that every filter type occurs"""
    from PIL import Image
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([(x * 3 + y * 2) & 255, (x * 5 + y) & 255, (x + y * 7) & 255, (x * 2 + y * 3) & 255], axis=-1).astype(np.uint8)
    base ^= (rng.integers(0, 4, (h, w, 4)) == 0).astype(np.uint8) * rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    kw = {}
    if kind == "grey":
        im = Image.fromarray(base[..., 0], "L")
    elif kind == "grey_key":
        im, kw = Image.fromarray(base[..., 0] & 0xF8, "L"), dict(transparency=int(base[3, 3, 0] & 0xF8))
    elif kind == "grey_alpha":
        im = Image.fromarray(base[..., :2], "LA")
    elif kind == "rgb":
        im = Image.fromarray(base[..., :3], "RGB")
    elif kind == "rgb_key":
        px = base[..., :3] & 0xC0
        im, kw = Image.fromarray(px, "RGB"), dict(transparency=tuple(int(v) for v in px[5, 5]))
    elif kind == "rgba":
        im = Image.fromarray(base, "RGBA")
    elif kind in ("palette", "palette_trns", "mask"):
        im = Image.fromarray((base[..., 0] >> 3) if kind == "mask" else base[..., 0], "P")
        im.putpalette(rng.integers(0, 256, 768, dtype=np.uint8).tobytes())
        if kind == "palette_trns":
            kw = dict(transparency=bytes(rng.integers(0, 256, 200, dtype=np.uint8)))
    else:
        raise ValueError(kind)
    buf = io.BytesIO()
    im.save(buf, "PNG", **kw)
    return buf.getvalue()


def sixteen_bit_file():
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray((np.arange(40 * 30, dtype=np.uint16) * 50).reshape(30, 40)).save(buf, "PNG")
    return buf.getvalue()


def alpha_plane(file):
    """the rule of include/fpng_amd.h: colour type 4 or 6, palette with a non-empty tRNS, grey with a tRNS of at least 2 bytes, RGB
    with one of at least 6"""
    color, at, trns = file[25], 33, 0
    while at + 12 <= len(file):
        n, kind = struct.unpack(">I4s", file[at:at + 8])
        if kind == b"IDAT":
            break
        if kind == b"tRNS":
            trns = n
        at += 12 + n
    return color in (4, 6) or (color == 3 and trns > 0) or (color == 0 and trns >= 2) or (color == 2 and trns >= 6)


def dims(file):
    return struct.unpack(">II", file[16:24])


def three_views(w, h):
    """(crop, full, window, filter, mirror) x 3: a 224-style downscale of a crop; an upscaled 16 x 16 crop whose box starts at
    (64, 64); a mirrored window with the bicubic filter"""
    return [((5, 7, w - 10, h - 12), (56, 56), None, "bilinear", False),
            ((64, 64, 16, 16), (40, 40), None, "bilinear", False),
            ((0, 0, w, h), (w // 2, h // 2), (10, 8, 32, 24), "bicubic", True)]


def to_device(files):
    import torch
    blob = torch.frombuffer(bytearray(b"".join(files)), dtype=torch.uint8).cuda()
    out, at = [], 0
    for f in files:
        out.append(blob[at:at + len(f)])
        at += len(f)
    return out


_ORACLE = {}


def oracle_file(enc, file):
    """decode_device_png of the file -- 4 channels when it has an alpha plane, else 3 -- encoded with the fpng encoder (made once per file)"""
    if file not in _ORACLE:
        c = 4 if alpha_plane(file) else 3
        (st, px, _), = enc.decode_device_png(to_device([file]), c)
        assert st == 0
        (png,), _ = enc.encode_tensors([px.contiguous()], 0)
        _ORACLE[file] = bytes(png)
    return _ORACLE[file]


def make_outs(views, chans, dtype, layout):
    import torch
    outs = []
    for (crop, full, window, _, _) in views:
        oh, ow = (window[3], window[2]) if window else (full[1], full[0])
        shape = (oh, ow, chans) if layout == "hwc" else (chans, oh, ow)
        outs.append(torch.full(shape, PATTERN, dtype=torch.uint8, device="cuda") if dtype is torch.uint8 else torch.full(shape, 7.0, dtype=dtype, device="cuda"))
    return outs


def untouched(t):
    import torch
    return bool((t == (PATTERN if t.dtype is torch.uint8 else 7.0)).all())


def run(enc, files, views, chans, dtype, layout, png=True, host=False, flags=0, **kw):
    """files[i] with views[i] (lists as three_views makes) into fresh pattern-filled destinations of chans[i] channels.
    png: the new call; else the existing views call of the layout.  -> (results, outs)"""
    import torch
    outs = [make_outs(v, c, dtype, layout) for v, c in zip(views, chans)]
    crops, full, window = [[v[0] for v in vs] for vs in views], [[v[1] for v in vs] for vs in views], [[v[2] for v in vs] for vs in views]
    filt, mirror = [[v[3] for v in vs] for vs in views], [[v[4] for v in vs] for vs in views]
    pngs = list(files) if host else to_device(files)
    if png:
        call = enc.decode_batch_png_views if host else enc.decode_device_png_views
        kw = dict(kw, layout=layout, flags=flags)
    else:
        call = {("planar", False): enc.decode_device_views, ("hwc", False): enc.decode_device_views_hwc, ("planar", True): enc.decode_batch_views, ("hwc", True): enc.decode_batch_views_hwc}[(layout, host)]
    res = call(pngs, crops, outs, full, window, filt, mirror, **kw)
    torch.cuda.synchronize()
    return res, outs


def same_as_oracle(enc, files, views, chans, dtype, layout, names=None, **kw):
    """the new call on the files against the existing call on their oracle files: status 0 and torch.equal, view by view"""
    import torch
    got, outs = run(enc, files, views, chans, dtype, layout, **kw)
    okw = {k: v for k, v in kw.items() if k not in ("host", "flags")}
    want, wouts = run(enc, [oracle_file(enc, f) for f in files], views, chans, dtype, layout, png=False, **okw)
    for i, ((st, _, _), (wst, _, _)) in enumerate(zip(got, want)):
        assert st == 0 and wst == 0, (names[i] if names else i, st, wst)
        for k, (a, b) in enumerate(zip(outs[i], wouts[i])):
            assert torch.equal(a, b), (names[i] if names else i, k, layout, dtype)
            assert not untouched(a)
    return got, outs


def routing_batch(enc):
    """(names, files, views, expected statuses): fpng-written files, Pillow-written ones, a marked file that the fast path answers
    NOT_FPNG, a 16-bit file, a truncated file, and a file with a crop outside"""
    import torch
    import fpng_amd
    names, files, views, want = [], [], [], []

    def add(name, f, vs, st):
        names.append(name), files.append(f), views.append(vs), want.append(st)

    fpng_files = []
    for k, c in enumerate((3, 4)):
        img = fpng_amd.synth_image(("grad", "blocks")[k], 130, 130, c)
        (png,), _ = enc.encode_tensors([torch.from_numpy(img).cuda()], 0)
        fpng_files.append(bytes(png))
    w, h = 130, 130
    add("fpng_rgb", fpng_files[0], three_views(w, h), 0)
    add("pillow_rgb", pillow_file("rgb", w, h, 11), three_views(w, h), 0)
    add("fpng_rgba", fpng_files[1], three_views(w, h)[:2], 0)
    add("pillow_palette_trns", pillow_file("palette_trns", w, h, 12), three_views(w, h), 0)
    marked = bytearray(fpng_files[0])  # (the marker chunk's version byte, its CRC made good: png_parse.h answers NOT_FPNG; an ancillary chunk to everyone else)
    assert marked[37:41] == b"fdEC" and marked[45] == 0
    marked[45] = 1
    marked[46:50] = struct.pack(">I", zlib.crc32(bytes(marked[37:46])))
    add("marked_not_fpng", bytes(marked), three_views(w, h)[:1], 0)
    add("sixteen_bit", sixteen_bit_file(), [((0, 0, 20, 20), (10, 10), None, "bilinear", False)], fpng_amd.FPNG_AMD_DECODE_UNSUPPORTED_PNG)
    add("truncated", pillow_file("rgba", w, h, 13)[:3000], three_views(w, h), None)
    add("crop_outside", pillow_file("grey", w, h, 14), [three_views(w, h)[0], ((100, 100, 31, 30), (8, 8), None, "bilinear", False)], fpng_amd.FPNG_AMD_DECODE_PNG_CROP_OUTSIDE)
    add("pillow_grey_alpha", pillow_file("grey_alpha", 200, 150, 15), three_views(200, 150), 0)
    add("fpng_crop_outside", fpng_files[0], [((0, 0, 131, 10), (8, 8), None, "bilinear", False)], fpng_amd.FPNG_AMD_DECODE_PNG_CROP_OUTSIDE)
    return names, files, views, want


def snapshot(res, outs):
    return [(st, c, [o.cpu().numpy().copy() for o in os_]) for (st, _, c), os_ in zip(res, outs)]


def _child():
    """one group against a file per group, in this fresh process; prints OK or fails"""
    import torch
    import fpng_amd
    enc = fpng_amd.Encoder(device=0)
    names, files, views, _ = routing_batch(enc)
    chans = [3] * len(files)
    flags = fpng_amd.FPNG_AMD_PNG_GENERAL_ONLY
    one = snapshot(*run(enc, files, views, chans, torch.uint8, "planar", flags=flags, post=fpng_amd.view_post(solarize=99), tone=fpng_amd.view_tone(autocontrast=True)))
    os.environ["FPNG_AMD_PNG_SCRATCH_LIMIT"] = "4096"  # (below every file's own need: a group per file)
    many = snapshot(*run(enc, files, views, chans, torch.uint8, "planar", flags=flags, post=fpng_amd.view_post(solarize=99), tone=fpng_amd.view_tone(autocontrast=True)))
    ok = sum(1 for a in one if a[0] == 0)
    assert ok >= 6, [a[0] for a in one]
    for name, a, b in zip(names, one, many):
        assert a[0] == b[0] and a[1] == b[1], (name, a[0], b[0])
        for x, y in zip(a[2], b[2]):
            assert np.array_equal(x, y), name
    enc.close()
    print("OK", ok)


BPP = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
UNDECIDED = 64


def small_views(w, h):
    """three_views for files from 80 x 48 up"""
    return [((5, 7, w - 10, h - 12), (56, 28), None, "bilinear", False),
            ((64, 32, 16, 16), (40, 40), None, "bilinear", False),
            ((0, 0, w, h), (w // 2, h // 2), (10, 8, 32, 24), "bicubic", True)]


def two_groups_batch(enc):
    """(names, files, views): files of 129 x 65 -- written by the fpng encoder, by Pillow, a marked file that the fpng path answers
    NOT_FPNG -- and tests/golden/first_pixel_match.png (65 x 16, RGBA), which it leaves UNDECIDED"""
    import torch
    import fpng_amd
    w, h = 129, 65
    fpng_files = []
    for k, c in enumerate((3, 4)):
        (png,), _ = enc.encode_tensors([torch.from_numpy(fpng_amd.synth_image(("grad", "blocks")[k], w, h, c)).cuda()], 0)
        fpng_files.append(bytes(png))
    marked = bytearray(fpng_files[0])  # (routing_batch's)
    assert marked[37:41] == b"fdEC" and marked[45] == 0
    marked[45] = 1
    marked[46:50] = struct.pack(">I", zlib.crc32(bytes(marked[37:46])))
    golden = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "first_pixel_match.png"), "rb").read()
    assert dims(golden) == (65, 16)
    batch = [("fpng_rgb", fpng_files[0], small_views(w, h)),
             ("pillow_rgb", pillow_file("rgb", w, h, 21), small_views(w, h)),
             ("marked_not_fpng", bytes(marked), small_views(w, h)[:1]),
             ("fpng_rgba", fpng_files[1], small_views(w, h)[:2]),
             ("pillow_palette_trns", pillow_file("palette_trns", w, h, 22), small_views(w, h)),
             ("first_pixel_match", golden, [((0, 0, 65, 16), (32, 8), None, "bilinear", False), ((40, 4, 16, 8), (24, 12), None, "bicubic", True)]),
             ("pillow_grey_alpha", pillow_file("grey_alpha", w, h, 23), small_views(w, h))]
    return [b[0] for b in batch], [b[1] for b in batch], [b[2] for b in batch]


def tier_need(file, views):
    """what a device-resident file of the general tier counts against FPNG_AMD_PNG_SCRATCH_LIMIT in the png_views calls, when no view
    has a post stage (the environment table; fpng_amd/csrc/png_tier_plan.h: png_groups): the scanlines it keeps, down
    to the last row of its box, rounded up to 256, and its share of the plan's scratch, the box's planes at 4 channels plus 256"""
    import fpng_amd
    w, _ = dims(file)
    _, by, bw, bh = fpng_amd.views_source([v[0] for v in views], [v[1] for v in views], [v[2] for v in views], [v[3] for v in views])
    up = lambda n, a: (n + a - 1) // a * a  # noqa: E731
    return up((by + bh) * (1 + w * BPP[file[25]]), 256) + up(up(bw * bh * 4, 16) + 256, 256)


def groups_of(needs, limit):
    """[g0, g1) of every group: a file joins while the sum stays at or under the limit; a file that alone exceeds it is a group of its own"""
    out, start, room = [], 0, 0
    for i, need in enumerate(needs):
        if i != start and room + need > limit:
            out.append((start, i))
            start, room = i, 0
        room += need
    return out + ([(start, len(needs))] if needs else [])


def _child_two_groups():
    """the small mixed batch, routed (flags 0): one group against exactly two with the UNDECIDED file in the second; prints OK or fails"""
    import torch
    import fpng_amd
    enc = fpng_amd.Encoder(device=0)
    names, files, views = two_groups_batch(enc)
    chans = [3] * len(files)
    fast = {"fpng_rgb", "fpng_rgba", "marked_not_fpng", "first_pixel_match"}
    for name, f in zip(names, files):
        assert (f[37:41] == b"fdEC") == (name in fast), name
    # the tier takes the files routed to it at once, in the call's order, then what the fpng path left, in the call's order
    order = [n for n in names if n not in fast] + ["marked_not_fpng", "first_pixel_match"]
    needs = [tier_need(files[names.index(n)], views[names.index(n)]) for n in order]
    limit = sum(needs[:3])  # (the three files routed at once fill the first group exactly: a sum equal to the limit joins)
    assert groups_of(needs, limit) == [(0, 3), (3, 5)] and groups_of(needs, 1 << 30) == [(0, 5)], (needs, limit)
    assert groups_of(needs, limit - 1)[0] == (0, 2)
    k = names.index("first_pixel_match")
    (st, _, _), = run(enc, [files[k]], [views[k]], [3], torch.uint8, "planar", png=False)[0]
    assert st == UNDECIDED, st
    one = snapshot(*run(enc, files, views, chans, torch.uint8, "planar"))
    os.environ["FPNG_AMD_PNG_SCRATCH_LIMIT"] = str(limit)
    two = snapshot(*run(enc, files, views, chans, torch.uint8, "planar"))
    assert [a[0] for a in one] == [0] * len(files), [a[0] for a in one]
    for name, a, b in zip(names, one, two):
        assert a[0] == b[0] and a[1] == b[1], (name, a[0], b[0])
        for x, y in zip(a[2], b[2]):
            assert np.array_equal(x, y) and not (x == PATTERN).all(), name
    enc.close()
    print("OK", limit)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    _child_two_groups() if sys.argv[1:] == ["two"] else _child()
