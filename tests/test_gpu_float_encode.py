"""GPU tests (-m gpu) of fpng_amd_encode_submit_planar_float: planar (CHW) device images of f32 / f16 / bf16 elements -- any
element-aligned base, any row and plane pitch of either sign, three planes of four -- quantised inside the row walk and encoded
where they lie.  The bar is test_gpu_layouts' judge (the reference's file, cpu_ref.ref() if built, else the oracle) for the bytes the
numpy ORACLE quantiser of test_float_encode_cpu gives for the very elements in memory; its generators keep every element 2^-10
away from a rounding tie (at most 1 % resampled, asserted there), and the ties themselves are test_float_encode_cpu's."""
import ctypes as C

import numpy as np
import pytest

from test_float_encode_cpu import IMAGENET_MEAN, IMAGENET_STD, element_values, float_image, oracle_quantize, subnormal_image, to_elements
from test_gpu_layouts import _check_gold, _content, _expect, _same

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 9), (3, 2), (63, 5), (64, 3), (65, 9), (255, 4), (256, 4), (257, 4), (512, 3), (1000, 17), (1001, 7), (7680, 4)]  # (w, h)
FLAGS = [0, 1, 2]  # 0, FPNG_ENCODE_SLOWER, FPNG_FORCE_UNCOMPRESSED
KINDS = ["contig", "wide", "odd", "neg", "rev", "far", "3of4"]
CODES = [0, 1, 2]  # FPNG_AMD_F32 / _F16 / _BF16
ELEM = {0: 4, 1: 2, 2: 2}
NP_BITS = {0: np.uint32, 1: np.uint16, 2: np.uint16}
NAN_BITS = {0: 0x7FC01234, 1: 0x7E55, 2: 0x7FC5}
INVALID_ARG, BUFFER_TOO_SMALL = -1, -4
_MEAN, _STD = IMAGENET_MEAN + (0.5,), IMAGENET_STD + (0.25,)


def _f32(v):
    return np.asarray(v, dtype=np.float64).astype(np.float32)


# how the floats are made of (byte + d) / 255 = u, and the constants that go with them:
#   unit: u itself, scale 255;  meanstd: (u - mean[c]) / std[c] with the inverse's constants;  clamp: u stretched to [-0.5, 1.5], scale
#   255, so that a quarter of the range clamps at either end
VARIANTS = {
    "unit": (None, _f32([255.0] * 4), _f32([0.0] * 4)),
    "meanstd": (lambda u, ch: (u - _MEAN[ch]) / _STD[ch], _f32([255.0 * s for s in _STD]), _f32([255.0 * m for m in _MEAN])),
    "clamp": (lambda u, ch: 2.0 * u - 0.5, _f32([255.0] * 4), _f32([0.0] * 4)),
}


@pytest.fixture(scope="module")
def enc(built_lib):
    import torch
    import fpng_amd
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    e = fpng_amd.Encoder(device=0)
    yield e
    e.close()


def _bits(el, code):
    return np.ascontiguousarray(el).view(NP_BITS[code])


def _planes(el, code, kind, fill=None):
    """test_gpu_planar's layouts counted in ELEMENTS: lays el (h, w, c) out as planes in one flat buffer of element bits -> (buffer,
    element offset of the R plane's top row, row pitch, plane pitch; both in elements).  kind: contig | wide (rows + 256) | odd (odd
    element offset, rows of w + 1: 16-bit rows start in the middle of a dword) | neg (bottom-up rows) | rev (planes in reverse order)
    | far (planes far apart) | 3of4 (a fourth plane behind the three that is not the image's).  Everything that is not a pixel is
    `fill`: None = zero, an int = that bit pattern, a generator = random bits."""
    h, w, c = el.shape
    bits = _bits(el, code)
    slots = 4 if kind == "3of4" else c
    ap = w + {"wide": 256, "odd": 1, "neg": 8}.get(kind, 0)
    app = h * ap + {"odd": 3, "rev": 5, "far": 100003}.get(kind, 0)
    front = 1 if kind == "odd" else 16
    total = front + slots * app + 16
    if fill is None or isinstance(fill, int):
        buf = np.full(total, fill or 0, dtype=bits.dtype)
    else:
        buf = fill.integers(0, 1 << (8 * bits.itemsize), total, dtype=np.uint64).astype(bits.dtype)

    def off(ch, r):
        return front + ((c - 1 - ch) if kind == "rev" else ch) * app + ((h - 1 - r) if kind == "neg" else r) * ap
    for ch in range(c):
        for r in range(h):
            buf[off(ch, r):off(ch, r) + w] = bits[r, :, ch]
    return buf, off(0, 0), (-ap if kind == "neg" else ap), (-app if kind == "rev" else app)


def _submit_raw(enc, descs, code, scale, bias, flags, reserved=0):
    """descs: list of (d_pixels, row_pitch, plane_pitch, w, h, num_chans, reserved, d_out, out_cap), pitches in bytes -> (rc, ticket)"""
    from fpng_amd import _lib
    arr = (_lib.ImagePlanar * len(descs))()
    for a, d in zip(arr, descs):
        a.d_pixels, a.row_pitch, a.plane_pitch, a.w, a.h, a.num_chans, a.reserved, a.d_out, a.out_cap = d
    fmt = _lib.FloatFormat()
    fmt.dtype, fmt.reserved = code, reserved
    for k in range(4):
        fmt.scale[k], fmt.bias[k] = float(scale[k]), float(bias[k])
    t = C.c_uint64(0)
    enc._sync_stream()
    rc = enc.lib.fpng_amd_encode_submit_planar_float(enc.h, arr, len(descs), C.byref(fmt), flags, C.byref(t))
    return rc, t.value


def _stage(cases, code, fill=None):
    """cases: list of (elements (h, w, c), kind) -> (descriptors, device buffers, host buffers, outputs)"""
    import torch
    import fpng_amd
    e = ELEM[code]
    descs, keep, bufs, outs = [], [], [], []
    for el, kind in cases:
        h, w, c = el.shape
        buf, top, rp, pp = _planes(el, code, kind, fill)
        d = torch.from_numpy(buf.view(np.uint8)).cuda()
        out = torch.empty(fpng_amd.max_encoded_size(w, h, c) + 64, dtype=torch.uint8, device="cuda")
        keep.append(d), bufs.append(buf), outs.append(out)
        descs.append((d.data_ptr() + top * e, rp * e, pp * e, w, h, c, 0, out.data_ptr(), out.numel()))
    return descs, keep, bufs, outs


def _collect(enc, t, keep, bufs, outs):
    res = enc.wait(t, len(outs))
    got = []
    for (size, mode, status), out in zip(res, outs):
        assert status == 0
        got.append((bytes(out[:size].cpu().numpy()), mode))
    for d, buf in zip(keep, bufs):  # the source, everything around the pixels included, is only read
        assert np.array_equal(d.cpu().numpy(), buf.view(np.uint8)), "submit_planar_float wrote into the source buffer"
    return got


def _run(enc, cases, code, scale, bias, flags, fill=None):
    """cases: list of (elements (h, w, c), kind) -> list of (file bytes, mode), ONE submission"""
    descs, keep, bufs, outs = _stage(cases, code, fill)
    rc, t = _submit_raw(enc, descs, code, scale, bias, flags)
    assert rc == 0, enc.lib.fpng_amd_last_error()
    return _collect(enc, t, keep, bufs, outs)


@pytest.fixture(scope="module")
def contents():
    return {(w, h, c): _content(i, w, h, c) for i, (w, h) in enumerate(SHAPES) for c in (3, 4)}


@pytest.fixture(scope="module")
def floats(contents):
    """(w, h, c, code, variant) -> (elements, the oracle's bytes), made once"""
    made = {}

    def get(w, h, c, code, variant):
        key = (w, h, c, code, variant)
        if key not in made:
            to_float, scale, bias = VARIANTS[variant]
            rng = np.random.default_rng([w, h, c, code, len(variant)])
            made[key] = float_image(contents[(w, h, c)], code, scale, bias, rng, to_float)
        return made[key]
    return get


@pytest.fixture(scope="module")
def expected():
    """the judge's file for (bytes, flags), made once per distinct image"""
    made = {}

    def get(by, flags):
        key = (by.shape, by.tobytes(), flags)
        if key not in made:
            made[key] = _expect(by, flags)
        return made[key]
    return get


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("code", CODES)
@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("c", [3, 4])
def test_parity_every_shape_and_layout(enc, floats, expected, c, flags, code, variant):
    _, scale, bias = VARIANTS[variant]
    kinds = [k for k in KINDS if not (k == "3of4" and c == 4)]
    cases, want = [], []
    for (w, h) in SHAPES:
        el, by = floats(w, h, c, code, variant)
        for k in kinds:
            cases.append((el, k))
            want.append(by)
    got = _run(enc, cases, code, scale, bias, flags, fill=np.random.default_rng(11))
    for (el, k), by, (png, mode) in zip(cases, want, got):
        _same(png, expected(by, flags), f"float code {code} {variant} c={c} {el.shape[1]}x{el.shape[0]} layout {k} flags {flags}")
        if flags == 2:
            assert mode == 1


def _sprinkle(el, code, rng):
    """NaN, +-inf, -0.0 and huge values in every plane, the first and the last pixel of rows included"""
    h, w, c = el.shape
    huge = 6.0e4 if code == 1 else 1.0e30
    special = to_elements([np.nan, np.inf, -np.inf, -0.0, huge, -huge], code)
    out = el.copy()
    for ch in range(c):
        for r in range(h):
            out[r, 0, ch] = special[(r + ch) % 6]
            out[r, w - 1, ch] = special[(r + ch + 3) % 6]
        ys, xs = rng.integers(0, h, 40), rng.integers(0, w, 40)
        out[ys, xs, ch] = special[rng.integers(0, 6, 40)]
    return out


@pytest.mark.parametrize("code", CODES)
def test_special_values(enc, floats, expected, code):
    rng = np.random.default_rng(17 + code)
    _, scale, bias = VARIANTS["meanstd"]
    for c in (3, 4):
        el = _sprinkle(floats(257, 4, c, code, "meanstd")[0], code, rng)
        x = element_values(el, code)
        by = np.stack([oracle_quantize(x[..., ch], scale[ch], bias[ch]) for ch in range(c)], axis=-1)
        assert (by[:, 0] == 0).any() and (by[:, -1] == 255).any()
        for flags in FLAGS:
            got = _run(enc, [(el, "contig"), (el, "odd"), (el, "neg")], code, scale, bias, flags)
            for (png, _), k in zip(got, ("contig", "odd", "neg")):
                _same(png, expected(by, flags), f"special values, code {code} c={c} layout {k} flags {flags}")


@pytest.mark.parametrize("code", [0, 1])
def test_subnormal_sources(enc, expected, code):
    """Images made of nothing but subnormal elements (test_float_encode_cpu.subnormal_image: every f16 subnormal with scale 2^22,
    fp32 subnormals with scale 2^127, exact ties among them), so a row's first and last pixel and every window interior hold one;
    w = 300 and w = 1300 so that both forms of the row walk run.  The device widens with the hardware's conversion where the host
    has a branch of its own: the file is the judge's for the rule's bytes in exact arithmetic -- a source flushed to zero would give
    an all-zero image."""
    for (w, h) in ((300, 9), (1300, 5)):
        for c in (3, 4):
            el, scale, bias, by = subnormal_image(code, w, h, c)
            assert by.any()
            for flags in FLAGS:
                got = _run(enc, [(el, "contig"), (el, "odd"), (el, "neg")], code, scale, bias, flags)
                for (png, _), k in zip(got, ("contig", "odd", "neg")):
                    _same(png, expected(by, flags), f"subnormal sources, code {code} {w}x{h}x{c} layout {k} flags {flags}")


@pytest.mark.parametrize("code", CODES)
@pytest.mark.parametrize("flags", FLAGS)
def test_nothing_but_pixels_matters(enc, floats, code, flags):
    """padding, gaps and the unused fourth plane filled with zeros and with NaN bit patterns: the same files (and, in _collect, an
    unchanged source)"""
    _, scale, bias = VARIANTS["meanstd"]
    cases = [(floats(w, h, c, code, "meanstd")[0], k) for c in (3, 4) for (w, h) in ((65, 9), (257, 4), (7680, 4))
             for k in ("wide", "odd", "far", "neg", "3of4") if not (k == "3of4" and c == 4)]
    zeros = _run(enc, cases, code, scale, bias, flags)
    nans = _run(enc, cases, code, scale, bias, flags, fill=NAN_BITS[code])
    for (el, k), a, b in zip(cases, zeros, nans):
        assert a == b, f"code {code} {el.shape} {k}: elements that are not pixels changed the file"


def test_refusals(enc, floats, expected):
    import torch
    import fpng_amd
    w, h = 65, 9
    one = _f32([255.0] * 4), _f32([0.0] * 4)
    for code in CODES:
        e = ELEM[code]
        el, by = floats(w, h, 4, code, "unit")
        src = torch.from_numpy(np.ascontiguousarray(_bits(el, code).transpose(2, 0, 1)).view(np.uint8).reshape(-1)).cuda()
        room = torch.zeros(src.numel() + 4096, dtype=torch.uint8, device="cuda")
        out = torch.empty(fpng_amd.max_encoded_size(w, h, 4) + 64, dtype=torch.uint8, device="cuda")
        cap, p, o, q = out.numel(), src.data_ptr(), out.data_ptr(), room.data_ptr()
        good = (p, 0, 0, w, h, 4, 0, o, cap)
        row, plane = w * e, h * w * e
        bad = {
            "misaligned base": (q + e // 2, 0, 0, w, h, 4, 0, o, cap),
            "misaligned row pitch": (q, row + e // 2, plane + 64 * e, w, h, 4, 0, o, cap),
            "misaligned plane pitch": (q, row, plane + e // 2, w, h, 4, 0, o, cap),
            "row pitch below the row": (p, row - e, plane, w, h, 4, 0, o, cap),
            "negative row pitch below the row": (p + (h - 1) * row, -(row - e), plane, w, h, 4, 0, o, cap),
            "planes overlap": (p, row, plane - e, w, h, 4, 0, o, cap),
            "negative plane pitch, planes overlap": (p + 3 * plane, row, -(plane - e), w, h, 4, 0, o, cap),
            "two channels": (p, 0, 0, w, h, 2, 0, o, cap),
            "image reserved not zero": (p, 0, 0, w, h, 4, 1, o, cap),
            "zero width": (p, 0, 0, 0, h, 4, 0, o, cap),
            "null pixels": (0, 0, 0, w, h, 4, 0, o, cap),
            "misaligned output": (p, 0, 0, w, h, 4, 0, o + 4, cap - 4),
        }
        if e == 4:
            bad["base two bytes off"] = (q + 2, 0, 0, w, h, 4, 0, o, cap)
        for what, d in bad.items():
            rc, t = _submit_raw(enc, [good, d], code, *one, 0)
            assert rc == INVALID_ARG and t == 0, f"code {code}, {what}: rc {rc}, ticket {t}"
        for what, kw in {"dtype 3": dict(code=3), "reserved = 1": dict(reserved=1)}.items():
            rc, t = _submit_raw(enc, [good], kw.get("code", code), *one, 0, reserved=kw.get("reserved", 0))
            assert rc == INVALID_ARG and t == 0, f"code {code}, {what}: rc {rc}, ticket {t}"
        for what, (sc, bi) in {"NaN scale": (_f32([255.0, float("nan"), 255.0, 255.0]), one[1]), "inf bias": (one[0], _f32([0.0, 0.0, 0.0, float("inf")]))}.items():
            rc, t = _submit_raw(enc, [good], code, sc, bi, 0)
            assert rc == INVALID_ARG and t == 0, f"code {code}, {what}: rc {rc}, ticket {t}"
        rc, t = _submit_raw(enc, [(p, 0, 0, w, h, 4, 0, o, fpng_amd.max_encoded_size(w, h, 4) - 1)], code, *one, 0)
        assert rc == BUFFER_TOO_SMALL and t == 0, "out_cap below max_encoded_size: as fpng_amd_encode_submit"
        # explicit pitches that equal the defaults, after all that
        out.zero_()
        rc, t = _submit_raw(enc, [(p, row, plane, w, h, 4, 0, o, cap)], code, *one, 0)
        assert rc == 0 and t
        (size, mode, status), = enc.wait(t, 1)
        assert status == 0
        _same(bytes(out[:size].cpu().numpy()), expected(by, 0), f"code {code}: valid submission after rejected ones")


def test_tickets_between_a_planar_and_a_packed_submission(enc, contents, floats, expected):
    """a float, a planar uint8 and a packed submission interleaved on one encoder, waited for out of order; the float one mixes
    channel counts and pitches"""
    import torch
    import fpng_amd
    from test_gpu_planar import _planes as _planes_u8, _submit_raw as _submit_raw_u8
    a3, a4 = contents[(1000, 17, 3)], contents[(65, 9, 4)]
    _, scale, bias = VARIANTS["meanstd"]
    for code in CODES:
        for flags in FLAGS:
            shapes = [(1000, 17, 3, "odd"), (65, 9, 4, "neg"), (257, 4, 3, "3of4"), (7680, 4, 4, "wide"), (512, 3, 4, "rev"), (1001, 7, 3, "far")]
            cases = [(floats(w, h, c, code, "meanstd")[0], k) for (w, h, c, k) in shapes]
            want = [floats(w, h, c, code, "meanstd")[1] for (w, h, c, k) in shapes]
            descs, keep, bufs, outs1 = _stage(cases, code, np.random.default_rng(3))
            rc, t1 = _submit_raw(enc, descs, code, scale, bias, flags)
            assert rc == 0 and t1
            # a planar uint8 submission behind it, NOT waited for yet
            pd, keep2, outs2 = [], [], []
            for img, kind in ((a3, "odd"), (a4, "rev")):
                h, w, c = img.shape
                buf, top, rp, pp = _planes_u8(img, kind, np.random.default_rng(4))
                d = torch.from_numpy(buf).cuda()
                out = torch.empty(fpng_amd.max_encoded_size(w, h, c) + 64, dtype=torch.uint8, device="cuda")
                keep2.append(d), outs2.append(out)
                pd.append((d.data_ptr() + top, rp, pp, w, h, c, 0, out.data_ptr(), out.numel()))
            rc, t2 = _submit_raw_u8(enc, pd, flags)
            assert rc == 0 and t2 == t1 + 1
            # ... and a packed one
            plain_in = [torch.from_numpy(a4).cuda(), torch.from_numpy(a3).cuda()]
            outs3 = [torch.empty(fpng_amd.max_encoded_size(i.shape[1], i.shape[0], i.shape[2]) + 64, dtype=torch.uint8, device="cuda") for i in plain_in]
            enc.submit(plain_in, outs3, flags)
            t3 = enc.last_ticket
            assert t3 == t2 + 1 and enc.query(t3) in (0, 1)
            r2, r3 = enc.wait(t2, 2), enc.wait(t3, 2)
            got1 = _collect(enc, t1, keep, bufs, outs1)
            for (el, k), by, (png, _) in zip(cases, want, got1):
                _same(png, expected(by, flags), f"float submission, code {code} {el.shape} {k} flags {flags}")
            for what, imgs, outs, res in (("planar", [a3, a4], outs2, r2), ("packed", [a4, a3], outs3, r3)):
                for img, out, (size, _, status) in zip(imgs, outs, res):
                    assert status == 0
                    _same(bytes(out[:size].cpu().numpy()), expected(img, flags), f"{what} submission next to a float one, flags {flags}")


@pytest.mark.parametrize("dtype", ["float32", "float16"])
def test_round_trip_with_the_float_decoder(enc, contents, dtype):
    """submit -> decode_device_float (ImageNet mean / std) -> submit_float (denormalize_constants of the same): the first file again.
    (bf16 is left out: its step at 255 is too close to half a byte to promise it.)"""
    import torch
    import fpng_amd
    for (w, h, c) in ((1000, 17, 3), (257, 4, 4)):
        img = contents[(w, h, c)]
        for flags in (0, 1):
            out = torch.empty(fpng_amd.max_encoded_size(w, h, c) + 64, dtype=torch.uint8, device="cuda")
            enc.submit([torch.from_numpy(img).cuda()], [out], flags)
            (size, _, status), = enc.wait(enc.last_ticket, 1)
            assert status == 0
            first = out[:size].clone()
            chw = torch.full((c, h, w), float("nan"), dtype=getattr(torch, dtype), device="cuda")
            (st, view, chans), = enc.decode_device_float([first], [chw], mean=IMAGENET_MEAN, std=IMAGENET_STD)
            assert st == 0 and chans == c
            out2 = torch.empty_like(out)
            enc.submit_float([chw], [out2], flags, mean=IMAGENET_MEAN, std=IMAGENET_STD)
            (size2, _, status), = enc.wait(enc.last_ticket, 1)
            assert status == 0
            _same(bytes(out2[:size2].cpu().numpy()), bytes(first.cpu().numpy()), f"round trip {dtype} {w}x{h}x{c} flags {flags}")


def test_torch_views_without_a_copy(enc):
    """nchw[i], a crop, [:3] of four planes, planes stored B, G, R and a bottom-up tensor through submit_float, against the
    reference on what torch's own chain gives for the same floats (values far from ties: (byte + 0.25) / 255)"""
    import torch
    import fpng_amd
    nchw8 = torch.stack([torch.from_numpy(fpng_amd.synth_image("blocks" if i & 1 else "grad", 701, 300, 4, seed=9 + i)).cuda().permute(2, 0, 1)
                         for i in range(3)]).contiguous()
    for dtype in (torch.float32, torch.float16):
        nchw = ((nchw8.to(torch.float32) + 0.25) / 255.0).to(dtype)
        cases = [
            (nchw[1], "rgba", False, nchw8[1]),
            (nchw[2][:, 37:250, 101:614], "rgba", False, nchw8[2][:, 37:250, 101:614]),
            (nchw[0][:3], "rgb", False, nchw8[0][:3]),
            (nchw[0][:3].flip(0).contiguous(), "bgr", False, nchw8[0][:3]),
            (nchw[1].flip(1).contiguous(), "rgba", True, nchw8[1]),
        ]
        views = [c[0] for c in cases]
        outs = [torch.empty(fpng_amd.max_encoded_size(v.shape[2], v.shape[1], v.shape[0]) + 64, dtype=torch.uint8, device="cuda") for v in views]
        enc.submit_float(list(views), outs, 0, order=[c[1] for c in cases], bottom_up=[c[2] for c in cases])
        res = enc.wait(enc.last_ticket, len(cases))
        for (v, order, up, want), out, (size, _, status) in zip(cases, outs, res):
            assert status == 0
            hwc = want.permute(1, 2, 0).contiguous().cpu().numpy()
            _same(bytes(out[:size].cpu().numpy()), _expect(hwc, 0), f"view {tuple(v.shape)} {v.dtype} {order} bottom_up={up}")
    with pytest.raises(ValueError):
        enc.submit_float([nchw[0].cpu()], [outs[0]])


def test_bench_set_from_f16_chw(enc):
    """The bench step (8 x 8K RGBA grad) held as f16 CHW tensors, bytes / 255: the committed reference digests."""
    import json
    import os
    import torch
    import fpng_amd
    from cpu_ref import ROOT
    with open(os.path.join(ROOT, "tests", "golden", "batches.json")) as f:
        s = json.load(f)["bench"]
    w, h, n = s["w"], s["h"], s["n"]
    need = n * (w * h * 4 * 2 + fpng_amd.max_encoded_size(w, h, 4)) + 3 * w * h * 4 * 4  # the f16 set, the outputs, the conversion's temporaries
    free = torch.cuda.mem_get_info()[0]
    if free < need + (4 << 30):
        pytest.skip(f"8 x 8K RGBA as f16 and its outputs need {need >> 20} MiB + scratch, {free >> 20} MiB are free")
    chw, outs = [], []
    for i in range(n):
        img = torch.from_numpy(fpng_amd.synth_image(s["kind"], w, h, 4, seed=s["seed0"] + i)).cuda()
        chw.append((img.permute(2, 0, 1).to(torch.float32) / 255.0).to(torch.float16).contiguous())
        del img
        outs.append(torch.empty(fpng_amd.max_encoded_size(w, h, 4) + 64, dtype=torch.uint8, device="cuda"))
    enc.submit_float(chw, outs, 0)
    _check_gold(enc.wait(enc.last_ticket, n), outs, s["flags"]["0"])
