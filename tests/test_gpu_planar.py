"""GPU tests (-m gpu) of fpng_amd_encode_submit_planar: planar (channels-first, CHW) device images -- any base byte, any row and
plane pitch of either sign, three planes of four -- encoded where they lie.  The bar is the file the reference writes for the same
pixels interleaved as R,G,B[,A] (test_gpu_layouts' judge: cpu_ref.ref() if built, else the oracle)."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_layouts import _check_gold, _content, _expect, _same, _submit_raw as _submit_raw_ex, _to_source, _layout, _fmt

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 9), (3, 2), (63, 5), (64, 3), (65, 9), (255, 4), (256, 4), (257, 4), (1000, 17), (1001, 7), (7680, 4)]  # (w, h)
FLAGS = [0, 1, 2]  # 0, FPNG_ENCODE_SLOWER, FPNG_FORCE_UNCOMPRESSED
KINDS = ["contig", "wide", "odd", "neg", "rev", "far", "3of4"]
INVALID_ARG, BUFFER_TOO_SMALL = -1, -4


@pytest.fixture(scope="module")
def enc(built_lib):
    import torch
    import fpng_amd
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    e = fpng_amd.Encoder(device=0)
    yield e
    e.close()


def _planes(img, kind, fill=None):
    """Lays img (h, w, c) R,G,B[,A] out as planes in one flat byte buffer -> (buffer, offset of the R plane's top row, row pitch,
    plane pitch).  kind: contig | wide (rows + 256) | odd (odd base, rows of w + 1) | neg (bottom-up rows) | rev (planes in reverse
    order, negative plane pitch) | far (planes far apart) | 3of4 (a fourth plane behind the three that is not the image's).
    Everything that is not a pixel comes from `fill` (a generator), or is zero."""
    h, w, c = img.shape
    slots = 4 if kind == "3of4" else c
    ap = w + {"wide": 256, "odd": 1, "neg": 8}.get(kind, 0)
    app = h * ap + {"odd": 3, "rev": 5, "far": 100003}.get(kind, 0)
    front = 1 if kind == "odd" else 16
    total = front + slots * app + 16
    buf = fill.integers(0, 256, total, dtype=np.uint8) if fill is not None else np.zeros(total, dtype=np.uint8)

    def off(ch, r):
        return front + ((c - 1 - ch) if kind == "rev" else ch) * app + ((h - 1 - r) if kind == "neg" else r) * ap
    for ch in range(c):
        for r in range(h):
            buf[off(ch, r):off(ch, r) + w] = img[r, :, ch]
    return buf, off(0, 0), (-ap if kind == "neg" else ap), (-app if kind == "rev" else app)


def _submit_raw(enc, descs, flags):
    """descs: list of (d_pixels, row_pitch, plane_pitch, w, h, num_chans, reserved, d_out, out_cap) -> (rc, ticket)"""
    from fpng_amd import _lib
    arr = (_lib.ImagePlanar * len(descs))()
    for a, d in zip(arr, descs):
        a.d_pixels, a.row_pitch, a.plane_pitch, a.w, a.h, a.num_chans, a.reserved, a.d_out, a.out_cap = d
    t = C.c_uint64(0)
    enc._sync_stream()
    rc = enc.lib.fpng_amd_encode_submit_planar(enc.h, arr, len(descs), flags, C.byref(t))
    return rc, t.value


def _run(enc, cases, flags, fill=None):
    """cases: list of (img (h, w, c), kind) -> list of (file bytes, mode), ONE submission"""
    import torch
    import fpng_amd
    descs, keep, outs, bufs = [], [], [], []
    for img, kind in cases:
        h, w, c = img.shape
        buf, top, rp, pp = _planes(img, kind, fill)
        d = torch.from_numpy(buf).cuda()
        out = torch.empty(fpng_amd.max_encoded_size(w, h, c) + 64, dtype=torch.uint8, device="cuda")
        keep.append(d)
        bufs.append(buf)
        outs.append(out)
        descs.append((d.data_ptr() + top, rp, pp, w, h, c, 0, out.data_ptr(), out.numel()))
    rc, t = _submit_raw(enc, descs, flags)
    assert rc == 0, enc.lib.fpng_amd_last_error()
    res = enc.wait(t, len(cases))
    got = []
    for (size, mode, status), out in zip(res, outs):
        assert status == 0
        got.append((bytes(out[:size].cpu().numpy()), mode))
    for d, buf in zip(keep, bufs):  # the source, everything around the pixels included, is only read
        assert np.array_equal(d.cpu().numpy(), buf), "submit_planar wrote into the source buffer"
    return got


@pytest.fixture(scope="module")
def contents():
    return {(w, h, c): _content(i, w, h, c) for i, (w, h) in enumerate(SHAPES) for c in (3, 4)}


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("c", [3, 4])
def test_parity_every_shape_and_layout(enc, contents, c, flags):
    kinds = [k for k in KINDS if not (k == "3of4" and c == 4)]
    cases = [(contents[(w, h, c)], k) for (w, h) in SHAPES for k in kinds]
    got = _run(enc, cases, flags, fill=np.random.default_rng(11))
    exp = {}
    for (img, k), (png, mode) in zip(cases, got):
        key = img.shape
        if key not in exp:
            exp[key] = _expect(img, flags)
        _same(png, exp[key], f"planar c={c} {img.shape[1]}x{img.shape[0]} layout {k} flags {flags}")
        if flags == 2:
            assert mode == 1


@pytest.mark.parametrize("flags", FLAGS)
def test_padding_gaps_and_an_unused_plane_do_not_matter(enc, contents, flags):
    cases = [(contents[(w, h, c)], k) for c in (3, 4) for (w, h) in ((65, 9), (257, 4), (7680, 4)) for k in ("wide", "odd", "far", "neg", "3of4")
             if not (k == "3of4" and c == 4)]
    zeros = _run(enc, cases, flags)
    noisy = _run(enc, cases, flags, fill=np.random.default_rng(5))
    for (img, k), a, b in zip(cases, zeros, noisy):
        assert a == b, f"{img.shape} {k}: bytes that are not pixels changed the file"


@pytest.fixture(scope="module")
def gold():
    import json
    import os
    from cpu_ref import ROOT
    with open(os.path.join(ROOT, "tests", "golden", "batches.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("flags", [0, 1])
def test_bench_set_from_chw(enc, gold, flags):
    """The bench step (8 x 8K RGBA grad) held as CHW tensors: the committed reference digests."""
    import torch
    import fpng_amd
    s = gold["bench"]
    w, h, n = s["w"], s["h"], s["n"]
    chw, outs = [], []
    for i in range(n):
        img = torch.from_numpy(fpng_amd.synth_image(s["kind"], w, h, 4, seed=s["seed0"] + i)).cuda()
        chw.append(img.permute(2, 0, 1).contiguous())
        del img
        outs.append(torch.empty(fpng_amd.max_encoded_size(w, h, 4) + 64, dtype=torch.uint8, device="cuda"))
    enc.submit_planar(chw, outs, flags)
    _check_gold(enc.wait(enc.last_ticket, n), outs, s["flags"][str(flags)])


def test_c3_set_from_nchw(enc, gold):
    """256 x 1080p RGB grad as ONE (n, 3, h, w) tensor, list(nchw) handed over: the committed reference digests."""
    import torch
    import fpng_amd
    s = gold["c3"]
    w, h, n = s["w"], s["h"], s["n"]
    nchw = torch.empty(n, 3, h, w, dtype=torch.uint8, device="cuda")
    for i in range(n):
        nchw[i].copy_(torch.from_numpy(fpng_amd.synth_image(s["kind"], w, h, 3, seed=s["seed0"] + i)).cuda().permute(2, 0, 1))
    outs = [torch.empty(fpng_amd.max_encoded_size(w, h, 3) + 64, dtype=torch.uint8, device="cuda") for _ in range(n)]
    enc.submit_planar(list(nchw), outs, 0)
    _check_gold(enc.wait(enc.last_ticket, n), outs, s["flags"]["0"])


def test_one_planar_submission_between_a_plain_and_an_ex_one(enc, contents):
    import torch
    import fpng_amd
    a3, a4 = contents[(1000, 17, 3)], contents[(65, 9, 4)]
    b4 = fpng_amd.synth_image("grad", 3840, 20, 4, seed=3)
    plain_in = [torch.from_numpy(a4).cuda(), torch.from_numpy(a3).cuda()]
    planar_cases = [(a3, "odd"), (a4, "neg"), (a3, "3of4"), (b4, "wide"), (a4, "rev"), (a3, "far"), (b4, "contig")]
    ex_cases = [(a3, "BGR", "odd"), (a4, "ARGB", "neg")]
    for flags in (0, 1, 2):
        out0 = [torch.empty(fpng_amd.max_encoded_size(i.shape[1], i.shape[0], i.shape[2]) + 64, dtype=torch.uint8, device="cuda") for i in plain_in]
        enc.submit(plain_in, out0, flags)
        t0 = enc.last_ticket
        # the planar submission: enqueued, NOT waited for yet
        descs, keep, outs1 = [], [], []
        for img, kind in planar_cases:
            h, w, c = img.shape
            buf, top, rp, pp = _planes(img, kind, np.random.default_rng(3))
            d = torch.from_numpy(buf).cuda()
            out = torch.empty(fpng_amd.max_encoded_size(w, h, c) + 64, dtype=torch.uint8, device="cuda")
            keep.append(d), outs1.append(out)
            descs.append((d.data_ptr() + top, rp, pp, w, h, c, 0, out.data_ptr(), out.numel()))
        rc, t1 = _submit_raw(enc, descs, flags)
        assert rc == 0 and t1 == t0 + 1
        # ... and an _ex one behind it
        exd, keep2, outs2 = [], [], []
        for img, name, pk in ex_cases:
            h, w, _ = img.shape
            v, _, c = _fmt(name)
            buf, top, pitch = _layout(_to_source(img, name, None), pk, None)
            d = torch.from_numpy(buf).cuda()
            out = torch.empty(fpng_amd.max_encoded_size(w, h, c) + 64, dtype=torch.uint8, device="cuda")
            keep2.append(d), outs2.append(out)
            exd.append((d.data_ptr() + top, pitch, w, h, v, out.data_ptr(), out.numel()))
        rc, t2 = _submit_raw_ex(enc, exd, flags)
        assert rc == 0 and t2 == t1 + 1
        assert enc.query(t2) in (0, 1)
        r2, r1, r0 = enc.wait(t2, len(exd)), enc.wait(t1, len(descs)), enc.wait(t0, 2)
        for what, imgs, outs, res in (("plain", [a4, a3], out0, r0), ("planar", [c[0] for c in planar_cases], outs1, r1),
                                      ("ex", [c[0] for c in ex_cases], outs2, r2)):
            for k, (img, out, (size, _, status)) in enumerate(zip(imgs, outs, res)):
                assert status == 0
                _same(bytes(out[:size].cpu().numpy()), _expect(img, flags), f"{what} submission, image {k}, flags {flags}")


def test_validation(enc, contents):
    import torch
    import fpng_amd
    img = contents[(65, 9, 4)]
    h, w, _ = img.shape
    src = torch.from_numpy(np.ascontiguousarray(img.transpose(2, 0, 1))).cuda()
    big = torch.from_numpy(np.random.default_rng(2).integers(0, 256, 4 * (h * (w + 1) + 3) + 64, dtype=np.uint8)).cuda()
    out = torch.empty(fpng_amd.max_encoded_size(w, h, 4) + 64, dtype=torch.uint8, device="cuda")
    cap = out.numel()
    p, o = src.data_ptr(), out.data_ptr()
    good = (p, 0, 0, w, h, 4, 0, o, cap)
    bad = {
        "row pitch below the row": (p, w - 1, h * w, w, h, 4, 0, o, cap),
        "negative row pitch below the row": (p + (h - 1) * w, -(w - 1), h * w, w, h, 4, 0, o, cap),
        "planes overlap": (p, w, (h - 1) * w + w - 1, w, h, 4, 0, o, cap),
        "negative plane pitch, planes overlap": (p + 3 * h * w, w, -(h * w - 1), w, h, 4, 0, o, cap),
        "planes overlap with padded rows": (p, w + 8, h * w, w, h, 3, 0, o, cap),
        "two channels": (p, 0, 0, w, h, 2, 0, o, cap),
        "five channels": (p, 0, 0, w, h, 5, 0, o, cap),
        "reserved not zero": (p, 0, 0, w, h, 4, 1, o, cap),
        "zero width": (p, 0, 0, 0, h, 4, 0, o, cap),
        "zero height": (p, 0, 0, w, 0, 4, 0, o, cap),
        "null pixels": (0, 0, 0, w, h, 4, 0, o, cap),
        "null output": (p, 0, 0, w, h, 4, 0, 0, cap),
        "misaligned output": (p, 0, 0, w, h, 4, 0, o + 4, cap - 4),
    }
    for what, d in bad.items():
        rc, t = _submit_raw(enc, [good, d], 0)
        assert rc == INVALID_ARG and t == 0, f"{what}: rc {rc}, ticket {t}"
    rc, t = _submit_raw(enc, [(p, 0, 0, w, h, 4, 0, o, fpng_amd.max_encoded_size(w, h, 4) - 1)], 0)
    assert rc == BUFFER_TOO_SMALL and t == 0, "out_cap below max_encoded_size: as fpng_amd_encode_submit"
    # four planes may start and be pitched at any byte (the file's content is whatever lies there)
    rc, t = _submit_raw(enc, [(big.data_ptr() + 1, w + 1, h * (w + 1) + 3, w, h, 4, 0, o, cap)], 0)
    assert rc == 0 and t
    enc.wait(t, 1)
    # explicit pitches that equal the defaults
    rc, t = _submit_raw(enc, [(p, w, h * w, w, h, 4, 0, o, cap)], 0)
    assert rc == 0 and t
    (size, mode, status), = enc.wait(t, 1)
    assert status == 0
    _same(bytes(out[:size].cpu().numpy()), _expect(img, 0), "explicit pitches")
    out.zero_()
    # after all that, a valid submission is right
    rc, t = _submit_raw(enc, [good], 0)
    assert rc == 0 and t
    (size, mode, status), = enc.wait(t, 1)
    assert status == 0
    _same(bytes(out[:size].cpu().numpy()), _expect(img, 0), "valid submission after rejected ones")


def test_torch_views_without_a_copy(enc):
    """nchw[i], a crop, [:3] of RGBA planes, flipped planes with order="bgr" and a bottom-up tensor through submit_planar, against
    the reference on the interleaved R,G,B[,A] pixels"""
    import torch
    import fpng_amd
    nchw = torch.stack([torch.from_numpy(fpng_amd.synth_image("blocks" if i & 1 else "grad", 701, 300, 4, seed=9 + i)).cuda().permute(2, 0, 1)
                        for i in range(3)]).contiguous()
    rgb = torch.from_numpy(fpng_amd.synth_image("grad", 333, 101, 3, seed=4)).cuda().permute(2, 0, 1).contiguous()
    cases = [
        (nchw[1], "rgba", False, nchw[1]),                                   # an image of a batch
        (nchw[2][:, 37:250, 101:614], "rgba", False, nchw[2][:, 37:250, 101:614]),  # crop: the parent's pitches, odd base
        (nchw[0][:3], "rgb", False, nchw[0][:3]),                            # RGBA planes -> RGB file
        (rgb.flip(0).contiguous(), "bgr", False, rgb),                       # planes stored B, G, R
        (nchw[1].flip(0).contiguous(), "abgr", False, nchw[1]),              # planes stored A, B, G, R
        (rgb.flip(1).contiguous(), "rgb", True, rgb),                        # bottom-up rows
    ]
    views = [c[0] for c in cases]
    outs = [torch.empty(fpng_amd.max_encoded_size(v.shape[2], v.shape[1], v.shape[0]) + 64, dtype=torch.uint8, device="cuda") for v in views]
    for flags in (0, 1, 2):
        enc.submit_planar(views, outs, flags, order=[c[1] for c in cases], bottom_up=[c[2] for c in cases])
        res = enc.wait(enc.last_ticket, len(cases))
        for (v, order, up, want), out, (size, _, status) in zip(cases, outs, res):
            assert status == 0
            hwc = want.permute(1, 2, 0).contiguous().cpu().numpy()
            _same(bytes(out[:size].cpu().numpy()), _expect(hwc, flags), f"view {tuple(v.shape)} {order} bottom_up={up} flags {flags}")
    with pytest.raises(ValueError):
        enc.submit_planar([rgb.cpu()], [outs[0]])
