"""GPU tests (-m gpu) of fpng_amd_encode_submit_ex: device images in other pixel layouts -- padded, odd and negative pitches,
BGR(A), ARGB / ABGR, padded alpha (*X / X*) -- encoded where they lie.  The bar is the file the reference writes for the same
pixels repacked as R,G,B[,A]."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

from cpu_ref import ROOT, fuzz_image, have_ref, oracle, ref

pytestmark = pytest.mark.gpu

FORMATS = ["RGB", "BGR", "RGBA", "BGRA", "ARGB", "ABGR", "RGBX", "BGRX", "XRGB", "XBGR"]
SHAPES = [(1, 1), (1, 9), (63, 5), (64, 3), (65, 9), (1000, 17), (7680, 4)]  # (w, h); 7680-pixel rows: the wide-row walk
FLAGS = [0, 1, 2]  # 0, FPNG_ENCODE_SLOWER, FPNG_FORCE_UNCOMPRESSED
INVALID_ARG, BUFFER_TOO_SMALL = -1, -4


@pytest.fixture(scope="module")
def enc(built_lib):
    import torch
    import fpng_amd
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    e = fpng_amd.Encoder(device=0)
    yield e
    e.close()


def _expect(img, flags):
    h, w, c = img.shape
    judge = ref() if have_ref() else oracle()
    return judge.encode(np.ascontiguousarray(img), w, h, c, flags)


def _fmt(name):
    import fpng_amd
    v, sb, c = fpng_amd.SRC_FORMATS[name]
    return v, sb, c


def _to_source(img, name, fill):
    """img (h, w, c) R,G,B[,A] -> source pixels (h, w, sb) of format `name`; X bytes from `fill` (a generator) or zero"""
    h, w, _ = img.shape
    _, sb, _ = _fmt(name)
    src = np.zeros((h, w, sb), dtype=np.uint8)
    for k, ch in enumerate(name):
        if ch == "X":
            src[..., k] = fill.integers(0, 256, (h, w), dtype=np.uint8) if fill is not None else 0
        else:
            src[..., k] = img[..., "RGBA".index(ch)]
    return src


def _layout(src, pitch_kind, fill=None):
    """Lays the source rows out in one flat byte buffer: returns (buffer bytes, offset of the top row's first byte, row pitch).
    pitch_kind: packed | odd (packed + 1, odd start byte) | wide (packed + 256) | neg (bottom-up, packed + 8)"""
    h, w, sb = src.shape
    packed = w * sb
    extra = {"packed": 0, "odd": 1, "wide": 256, "neg": 8}[pitch_kind]
    ap = packed + extra
    front = 1 if pitch_kind == "odd" else 16  # (16 bytes of guard in front, 4-byte aligned)
    total = front + h * ap + 16
    buf = fill.integers(0, 256, total, dtype=np.uint8) if fill is not None else np.zeros(total, dtype=np.uint8)
    for r in range(h):
        row = (h - 1 - r) if pitch_kind == "neg" else r
        o = front + row * ap
        buf[o:o + packed] = src[r].reshape(-1)
    top = front + ((h - 1) * ap if pitch_kind == "neg" else 0)
    return buf, top, (-ap if pitch_kind == "neg" else ap)


def _content(i, w, h, c):
    import fpng_amd
    kind = i % 3
    if kind == 0:
        return fuzz_image(np.random.default_rng(1000 + i), force_dims=(w, h), c=c)[0]
    return fpng_amd.synth_image("grad" if kind == 1 else "blocks", w, h, c, seed=77 + i)


def _submit_raw(enc, descs, flags):
    """descs: list of (d_pixels, row_pitch, w, h, format, d_out, out_cap) -> (rc, ticket)"""
    from fpng_amd import _lib
    arr = (_lib.ImageEx * len(descs))()
    for a, d in zip(arr, descs):
        a.d_pixels, a.row_pitch, a.w, a.h, a.format, a.d_out, a.out_cap = d
    t = C.c_uint64(0)
    enc._sync_stream()
    rc = enc.lib.fpng_amd_encode_submit_ex(enc.h, arr, len(descs), flags, C.byref(t))
    return rc, t.value


def _run(enc, cases, flags, fill=None):
    """cases: list of (img (h, w, c) R,G,B[,A], format name, pitch kind) -> list of (file bytes, mode), one submission"""
    import torch
    import fpng_amd
    descs, keep, outs, bufs = [], [], [], []
    for img, name, pk in cases:
        h, w, _ = img.shape
        v, _, c = _fmt(name)
        buf, top, pitch = _layout(_to_source(img, name, fill), pk, fill)
        d = torch.from_numpy(buf).cuda()
        out = torch.empty(fpng_amd.max_encoded_size(w, h, c) + 64, dtype=torch.uint8, device="cuda")
        keep.append(d)
        bufs.append(buf)
        outs.append(out)
        descs.append((d.data_ptr() + top, pitch, w, h, v, out.data_ptr(), out.numel()))
    rc, t = _submit_raw(enc, descs, flags)
    assert rc == 0, enc.lib.fpng_amd_last_error()
    res = enc.wait(t, len(cases))
    got = []
    for (size, mode, status), out in zip(res, outs):
        assert status == 0
        got.append((bytes(out[:size].cpu().numpy()), mode))
    for d, buf in zip(keep, bufs):  # the source, padding and X bytes included, is only read
        assert np.array_equal(d.cpu().numpy(), buf), "submit_ex wrote into the source buffer"
    return got


def _same(png, exp, what):
    if png != exp:
        n = min(len(png), len(exp))
        x = np.frombuffer(png[:n], np.uint8) != np.frombuffer(exp[:n], np.uint8)
        d = int(np.argmax(x)) if x.any() else n
        raise AssertionError(f"{what}: sizes {len(png)} vs {len(exp)}, first difference at byte {d}")


@pytest.fixture(scope="module")
def contents():
    return {(w, h, c): _content(i, w, h, c) for i, (w, h) in enumerate(SHAPES) for c in (3, 4)}


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("name", FORMATS)
def test_parity_every_format_shape_and_pitch(enc, contents, name, flags):
    _, sb, c = _fmt(name)
    kinds = ["packed", "wide", "neg"] + (["odd"] if sb == 3 else [])
    cases = [(contents[(w, h, c)], name, pk) for (w, h) in SHAPES for pk in kinds]
    got = _run(enc, cases, flags)
    exp = {}
    for (img, _, pk), (png, mode) in zip(cases, got):
        key = img.shape
        if key not in exp:
            exp[key] = _expect(img, flags)
        _same(png, exp[key], f"{name} {img.shape[1]}x{img.shape[0]} pitch {pk} flags {flags}")
        if flags == 2:
            assert mode == 1


@pytest.mark.parametrize("flags", [0, 1, 2])
def test_padding_and_x_bytes_do_not_matter(enc, contents, flags):
    rng = np.random.default_rng(5)
    cases = [(contents[(w, h, _fmt(n)[2])], n, pk) for n in ("BGRX", "XRGB", "ABGR", "BGR") for (w, h) in ((65, 9), (7680, 4))
             for pk in ("wide", "neg")]
    zeros = _run(enc, cases, flags)
    noisy = _run(enc, cases, flags, fill=rng)
    for (img, n, pk), a, b in zip(cases, zeros, noisy):
        assert a == b, f"{n} {img.shape} {pk}: padding / X bytes changed the file"


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(ROOT, "tests", "golden", "batches.json")) as f:
        return json.load(f)


def _check_gold(res, outs, exp):
    for i, (size, mode, status) in enumerate(res):
        assert status == 0 and mode == 0
        assert size == exp["sizes"][i]
        assert hashlib.sha256(outs[i][:size].cpu().numpy().tobytes()).hexdigest() == exp["sha256"][i], f"image {i} differs"


@pytest.mark.parametrize("flags", [0, 1])
def test_bench_set_as_padded_bgra(enc, gold, flags):
    """The bench step (8 x 8K RGBA grad) laid out as BGRA rows of w*4 + 256 bytes: the committed reference digests."""
    import torch
    import fpng_amd
    s = gold["bench"]
    w, h, n = s["w"], s["h"], s["n"]
    views, outs = [], []
    for i in range(n):
        img = torch.from_numpy(fpng_amd.synth_image(s["kind"], w, h, 4, seed=s["seed0"] + i)).cuda()
        buf = torch.randint(0, 256, (h, w * 4 + 256), dtype=torch.uint8, device="cuda")
        v = buf[:, :w * 4].view(h, w, 4)
        v.copy_(img[..., [2, 1, 0, 3]])
        del img
        views.append(v)
        outs.append(torch.empty(fpng_amd.max_encoded_size(w, h, 4) + 64, dtype=torch.uint8, device="cuda"))
    enc.submit_ex(views, outs, flags, order="bgra")
    _check_gold(enc.wait(enc.last_ticket, n), outs, s["flags"][str(flags)])


def test_c3_set_as_bgr_and_as_rgbx(enc, gold):
    """256 x 1080p RGB grad, once as BGR and once as RGB in 4-byte pixels: the committed reference digests."""
    import torch
    import fpng_amd
    s = gold["c3"]
    w, h, n = s["w"], s["h"], s["n"]
    imgs = [torch.from_numpy(fpng_amd.synth_image(s["kind"], w, h, 3, seed=s["seed0"] + i)).cuda() for i in range(n)]
    outs = [torch.empty(fpng_amd.max_encoded_size(w, h, 3) + 64, dtype=torch.uint8, device="cuda") for _ in range(n)]
    bgr = [im[..., [2, 1, 0]].contiguous() for im in imgs]
    enc.submit_ex(bgr, outs, 0, order="bgr")
    _check_gold(enc.wait(enc.last_ticket, n), outs, s["flags"]["0"])
    del bgr
    rgbx = []
    for im in imgs:
        q = torch.full((h, w, 4), 0xA5, dtype=torch.uint8, device="cuda")
        q[..., :3] = im
        rgbx.append(q[..., :3])
    del imgs
    for o in outs:
        o.zero_()
    enc.submit_ex(rgbx, outs, 0)
    _check_gold(enc.wait(enc.last_ticket, n), outs, s["flags"]["0"])


def test_one_mixed_submission_between_plain_ones(enc, contents):
    import torch
    import fpng_amd
    a3, a4 = contents[(1000, 17, 3)], contents[(65, 9, 4)]
    b4 = fpng_amd.synth_image("grad", 3840, 20, 4, seed=3)
    plain_in = [torch.from_numpy(a4).cuda(), torch.from_numpy(a3).cuda()]

    def outs_for(ims):
        return [torch.empty(fpng_amd.max_encoded_size(i.shape[1], i.shape[0], i.shape[2]) + 64, dtype=torch.uint8, device="cuda")
                for i in ims]
    ex_cases = [(a3, "BGR", "odd"), (a4, "ARGB", "neg"), (a3, "XBGR", "wide"), (b4, "BGRA", "wide"), (a4, "RGBA", "packed"),
                (a3, "RGBX", "neg")]
    for flags in (0, 1):
        out0, out2 = outs_for(plain_in), outs_for(plain_in[::-1])  # (buffers of submissions in flight must not alias)
        enc.submit(plain_in, out0, flags)
        t0 = enc.last_ticket
        got = _run(enc, ex_cases, flags)  # (waits for its own ticket only)
        enc.submit(plain_in[::-1], out2, flags)
        t2 = enc.last_ticket
        r2, r0 = enc.wait(t2, 2), enc.wait(t0, 2)
        for (img, n, pk), (png, _) in zip(ex_cases, got):
            _same(png, _expect(img, flags), f"mixed {n} {pk} flags {flags}")
        for imgs, outs, res in (([a4, a3], out0, r0), ([a3, a4], out2, r2)):
            for img, out, (size, _, status) in zip(imgs, outs, res):
                assert status == 0
                _same(bytes(out[:size].cpu().numpy()), _expect(img, flags), "plain submission around the mixed one")


def test_validation(enc, contents):
    import torch
    import fpng_amd
    img = contents[(65, 9, 4)]
    h, w, _ = img.shape
    src = torch.from_numpy(np.ascontiguousarray(_to_source(img, "BGRA", None))).cuda()
    big = torch.zeros(w * h * 4 + 64, dtype=torch.uint8, device="cuda")
    out = torch.empty(fpng_amd.max_encoded_size(w, h, 4) + 64, dtype=torch.uint8, device="cuda")
    cap = out.numel()
    p, o = src.data_ptr(), out.data_ptr()
    BGRA, BGR, XRGB = _fmt("BGRA")[0], _fmt("BGR")[0], _fmt("XRGB")[0]
    good = (p, 0, w, h, BGRA, o, cap)
    bad = {
        "unknown format": (p, 0, w, h, 10, o, cap),
        "pitch below the row": (p, w * 4 - 4, w, h, BGRA, o, cap),
        "negative pitch below the row": (p + (h - 1) * w * 4, -(w * 4 - 1), w, h, BGRA, o, cap),
        "3-byte pitch below the row": (p, w * 3 - 1, w, h, BGR, o, cap),
        "misaligned 4-byte base": (big.data_ptr() + 2, 0, w, h, BGRA, o, cap),
        "misaligned 4-byte pitch": (p, w * 4 + 2, w, h, XRGB, o, cap),
        "zero width": (p, 0, 0, h, BGRA, o, cap),
        "zero height": (p, 0, w, 0, BGRA, o, cap),
        "null pixels": (0, 0, w, h, BGRA, o, cap),
        "null output": (p, 0, w, h, BGRA, 0, cap),
        "misaligned output": (p, 0, w, h, BGRA, o + 4, cap - 4),
    }
    for what, d in bad.items():
        rc, t = _submit_raw(enc, [good, d], 0)
        assert rc == INVALID_ARG and t == 0, f"{what}: rc {rc}, ticket {t}"
    rc, t = _submit_raw(enc, [(p, 0, w, h, BGRA, o, fpng_amd.max_encoded_size(w, h, 4) - 1)], 0)
    assert rc == BUFFER_TOO_SMALL and t == 0, "out_cap below max_encoded_size: as fpng_amd_encode_submit"
    # 3-byte sources may start and be pitched at any byte
    rc, t = _submit_raw(enc, [(big.data_ptr() + 1, w * 3 + 1, w, h, BGR, o, cap)], 0)
    assert rc == 0 and t
    enc.wait(t, 1)
    # after all that, a valid submission is right
    rc, t = _submit_raw(enc, [good], 0)
    assert rc == 0 and t
    (size, mode, status), = enc.wait(t, 1)
    assert status == 0
    _same(bytes(out[:size].cpu().numpy()), _expect(img, 0), "valid submission after rejected ones")


def test_torch_views_without_a_copy(enc):
    """A crop, a [..., :3] slice of RGBA, a cv2-style BGR frame and a bottom-up buffer through submit_ex, against the reference on
    .contiguous() of the R,G,B[,A] version"""
    import torch
    import fpng_amd
    big = torch.from_numpy(fpng_amd.synth_image("blocks", 700, 300, 4, seed=9)).cuda()
    rgb = torch.from_numpy(fpng_amd.synth_image("grad", 333, 101, 3, seed=4)).cuda()
    cases = [
        (big[37:250, 101:613], "rgba", False, big[37:250, 101:613]),      # crop
        (big[:, 3:517, :3], "rgb", False, big[:, 3:517, :3]),            # RGBA -> RGB
        (rgb[..., [2, 1, 0]].contiguous(), "bgr", False, rgb),           # cv2-style BGR
        (big[10:90, 5:405, 1:], "bgr", False, big[10:90, 5:405, 1:].flip(2)),  # [..., 1:] of 4-byte pixels read as BGR: XBGR
        (rgb.flip(0).contiguous(), "rgb", True, rgb),                     # GL-style bottom-up
    ]
    views = [c[0] for c in cases]
    outs = [torch.empty(fpng_amd.max_encoded_size(v.shape[1], v.shape[0], v.shape[2]) + 64, dtype=torch.uint8, device="cuda")
            for v in views]
    for flags in (0, 1):
        enc.submit_ex(views, outs, flags, order=[c[1] for c in cases], bottom_up=[c[2] for c in cases])
        res = enc.wait(enc.last_ticket, len(cases))
        for (v, order, up, want), out, (size, _, status) in zip(cases, outs, res):
            assert status == 0
            _same(bytes(out[:size].cpu().numpy()), _expect(want.contiguous().cpu().numpy(), flags), f"view {order} bottom_up={up}")
