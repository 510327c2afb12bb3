"""GPU decoder of a WINDOW of each file's crop resized to a fixed size, bilinear or bicubic, optionally mirrored (-m gpu;
fpng_amd_decode_batch_planar_resize_view / fpng_amd_decode_batch_device_planar_resize_view: the crop kernels decode the box the
window's taps reach into the decode scratch, then dec_resize_kernel): uint8 planes and the three float dtypes, three and four planes,
mirror off and on, both filters, every pitch kind, host and device files.

Expected values never come from the library: the pixels are the REFERENCE's decoder's (judge()), sliced to the crop, resized WHOLE
and sliced to the window by resize_view_model.py (test_resize_view_cpu.py pins that text to Pillow), and for the float dtypes looked
up in test_gpu_decode_float's table.  Buffers are sentinel-filled and compared WHOLE and bit for bit.

The views (resize_view_model.VIEWS) are the smallest shapes at which the kernel can go wrong: windows that start inside the full
image (weights at x + i, taps outside the window's pre-image), a box that starts past the first tile of the pixel pass (addressing
relative to the box), the far corner one past a 64 x 16 tile (taps clipped at the crop's edge), both scale limits, 1 x 1 windows."""
import numpy as np
import pytest

from test_gpu_decode import UNDECIDED, _device_files
from test_gpu_decode_float import CONSTS
from test_gpu_decode_layouts import SENTINEL, _damaged_files, _header_dims
from test_gpu_decode_planar import KINDS
from test_gpu_decode_resize import BITS, CROP_OUTSIDE, DTYPES, ELEM, _elements, _expect, _first_difference, _regions, enc, files  # noqa: F401  (enc, files: fixtures)
import resize_view_model as VM

pytestmark = pytest.mark.gpu


def _window(full, window):
    return (0, 0) + tuple(full) if window is None else tuple(window)


class _Model:
    """the model's bytes of (file, crop, full, filter), resized whole once each from the reference decoder's four planes; a view is a slice"""

    def __init__(self, files):
        self.files, self._full = files, {}

    def view(self, i, crop, full, window, filter):
        """(4, h, w) uint8 of the window, not mirrored"""
        key = (i, crop, full, filter)
        if key not in self._full:
            x, y, w, h = crop
            r = VM.view_planes(self.files.planes[i][:, y:y + h, x:x + w], full, None, filter)
            r.setflags(write=False)
            self._full[key] = r
        x, y, w, h = _window(full, window)
        return self._full[key][:, y:y + h, x:x + w]


@pytest.fixture(scope="module")
def model(files):  # noqa: F811
    return _Model(files)


def _cases(files, filter):  # noqa: F811
    """(file, crop, full, window) of every file x every view of its size that runs with this filter"""
    return [(i, crop, full, window) for i, d in enumerate(files.dims) for crop, full, window, fs in VM.VIEWS[d] if filter in fs]


def _decode_view(enc, pngs, crops, fulls, windows, filters, regs, total, dtype, device, mirror, consts=CONSTS[0], dev=None):  # noqa: F811
    """one call into ONE sentinel-filled buffer of `total` elements: (results, the elements' bits afterwards, the views)"""
    import torch
    e = ELEM[dtype]
    buf = torch.full((total * e,), SENTINEL, dtype=torch.uint8, device="cuda")
    typed = buf.view(getattr(torch, dtype))
    views = [typed.as_strided((r.c, r.h, r.w), (r.pp, r.rp, 1), r.lo) for r in regs]
    orders, ups = [r.order() for r in regs], [r.kind == "bottom_up" for r in regs]
    kw = {} if dtype == "uint8" else {"scale": consts[0], "bias": consts[1]}
    if device:
        got = enc.decode_device_resize_view(dev if dev is not None else _device_files(pngs, shift=1), crops, views, fulls, windows, filters, mirror=mirror, order=orders,
                                            bottom_up=ups, **kw)
    else:
        got = enc.decode_batch_resize_view(pngs, crops, views, fulls, windows, filters, mirror=mirror, order=orders, bottom_up=ups, **kw)
    torch.cuda.synchronize()
    return got, buf.cpu().numpy().view(BITS[e]), views


def _run_cases(enc, files, model, cases, filters, c, dtype, device, mirrors, kinds):  # noqa: F811
    crops, fulls, windows = [k[1] for k in cases], [k[2] for k in cases], [k[3] for k in cases]
    regs, total = _regions([_window(f, w)[2:] for f, w in zip(fulls, windows)], c, kinds)
    got, host, views = _decode_view(enc, [files.pngs[k[0]] for k in cases], crops, fulls, windows, filters, regs, total, dtype, device, mirrors)
    for k, ((i, *_), (st, view, cf)) in enumerate(zip(cases, got)):
        assert st == 0 and cf == files.chans[i] and view is views[k], (k, i, st, cf)
    exp = _expect(total, dtype, regs, [_elements(model.view(*case, f), c, dtype, m) for case, f, m in zip(cases, filters, mirrors)])
    diff = _first_difference(host, exp, regs)
    assert diff is None, (c, dtype, device, diff, [(cases[j], filters[j]) for j, *_ in diff[4]])


@pytest.mark.parametrize("filter", VM.FILTERS)
@pytest.mark.parametrize("mirror", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", [3, 4])
def test_view_matrix_device_files(enc, files, model, c, dtype, mirror, filter):  # noqa: F811
    """every file x every view of its size, into three and four planes of every dtype, mirror off and on, in either filter, pitch
    kinds dealt round-robin: ONE call into ONE buffer that is compared whole"""
    cases = _cases(files, filter)
    kinds = [KINDS[(k + c) % len(KINDS)] for k in range(len(cases))]
    _run_cases(enc, files, model, cases, [filter] * len(cases), c, dtype, True, [mirror] * len(cases), kinds)


@pytest.mark.parametrize("c,dtype,mirror,filter", [(3, "uint8", True, "bicubic"), (4, "bfloat16", False, "bilinear"), (4, "float32", True, "bicubic")])
def test_view_matrix_host_files(enc, files, model, c, dtype, mirror, filter):  # noqa: F811
    """the same through fpng_amd_decode_batch_planar_resize_view (files in host memory), for a subset"""
    cases = _cases(files, filter)[::2]
    kinds = [KINDS[(k + 2 * c) % len(KINDS)] for k in range(len(cases))]
    _run_cases(enc, files, model, cases, [filter] * len(cases), c, dtype, False, [mirror] * len(cases), kinds)


def test_the_whole_bilinear_window_is_the_plain_resize_call(enc, files):  # noqa: F811
    """600 x 130 -> 224 x 224, no window, bilinear: byte for byte what decode_device_resize writes, mirrored or not, bytes and f16"""
    import torch
    idx = [i for i, d in enumerate(files.dims) if d == (600, 130)]
    dev = _device_files([files.pngs[i] for i in idx])
    crops = [(0, 0, 600, 130)] * len(idx)
    mirrors = [bool(k & 1) for k in range(len(idx))]
    for dtype, kw in ((torch.uint8, {}), (torch.float16, {"mean": (0.485, 0.456, 0.406), "std": (0.229, 0.224, 0.225)})):
        a = torch.full((len(idx), 3, 224, 224), 7, dtype=dtype, device="cuda")
        b = torch.full((len(idx), 3, 224, 224), 9, dtype=dtype, device="cuda")
        got_a = enc.decode_device_resize(dev, crops, list(a), mirror=mirrors, **kw)
        got_b = enc.decode_device_resize_view(dev, crops, list(b), (224, 224), mirror=mirrors, **kw)
        torch.cuda.synchronize()
        assert [st for st, _, _ in got_a] == [st for st, _, _ in got_b] == [0] * len(idx)
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), dtype
    got = enc.decode_device_resize_view(dev, crops, full=(256, 256), window=(16, 16, 224, 224), filter="bicubic", dtype=torch.float16)  # (outs=None allocates)
    assert all(st == 0 and v.dtype == torch.float16 and tuple(v.shape) == (3, 224, 224) for st, v, _ in got)


def _mixed(files):  # noqa: F811
    """a batch of twelve: both filters, windows, mirrors, 3- and 4-channel files, stored files; file 4's crop leaves the image"""
    rng = np.random.default_rng(31)
    both = [(case, f) for f in VM.FILTERS for case in _cases(files, f)]
    pick = [both[int(v)] for v in rng.permutation(len(both))[:12]]
    i4 = pick[4][0][0]
    pick[4] = ((i4, (files.dims[i4][0] - 1, 0, 2, 1), (7, 5), (1, 1, 5, 3)), "bicubic")
    assert {f for _, f in pick} == set(VM.FILTERS) and {files.chans[k[0]] for k, _ in pick} == {3, 4}
    assert any(k[3] is not None for k, _ in pick) and any(files.dims[k[0]] != (600, 130) for k, _ in pick)
    # (a stored file holds its pixels and a filter byte per row uncompressed: it is longer than they are)
    assert any(len(files.pngs[k[0]]) > files.dims[k[0]][0] * files.dims[k[0]][1] * files.chans[k[0]] for n, (k, _) in enumerate(pick) if n != 4)
    return pick, [bool(v) for v in rng.integers(0, 2, 12)]


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("dtype", ["uint8", "float16"])
def test_one_mixed_batch(enc, files, model, dtype, device):  # noqa: F811
    """Twelve clean files and one damaged one in ONE call.  The file whose crop leaves the image gets status 67 and its region stays
    untouched; the damaged file gets the status the CROP call gives it for its box (a whole window: the crop itself), and nothing
    outside its spans is written; every other file is exact."""
    pick, mirrors = _mixed(files)
    damaged = None
    for p in _damaged_files():
        w, h = _header_dims(p)
        if not (1 <= w <= 600 and 1 <= h <= 600):
            continue
        crop = (0, max(h - 2, 0), w, min(h, 2))
        (st, _, _), = enc.decode_batch_crop([p], [crop])
        if st not in (0, UNDECIDED):
            damaged = (p, crop, (max(w // 3, 1), 3), st)
            break
    assert damaged is not None
    pngs = [files.pngs[k[0]] for k, _ in pick] + [damaged[0]]
    crops = [k[1] for k, _ in pick] + [damaged[1]]
    fulls = [k[2] for k, _ in pick] + [damaged[2]]
    windows = [k[3] for k, _ in pick] + [None]
    filters = [f for _, f in pick] + ["bicubic"]
    mirrors = mirrors + [True]
    c = 3
    kinds = [KINDS[k % len(KINDS)] for k in range(len(pngs))]
    regs, total = _regions([_window(f, w)[2:] for f, w in zip(fulls, windows)], c, kinds)
    got, host, _ = _decode_view(enc, pngs, crops, fulls, windows, filters, regs, total, dtype, device, mirrors)
    sts = [st for st, _, _ in got]
    assert sts == [0] * 4 + [CROP_OUTSIDE] + [0] * 7 + [damaged[3]], sts
    sources = [None if k == 4 else _elements(model.view(*case, f), c, dtype, mirrors[k]) for k, (case, f) in enumerate(pick)] + [None]
    exp = _expect(total, dtype, regs, sources)
    for a, b in regs[12].spans():  # (what a rejected file's spans hold is not defined)
        exp[a:b] = host[a:b]
    assert _first_difference(host, exp, regs) is None, _first_difference(host, exp, regs)


@pytest.mark.parametrize("device", [False, True])
def test_checksums_verified(enc, files, model, device):  # noqa: F811
    """set_decode_verify(CRC-32 and Adler-32): every tile of every file runs under the Adler-32 check while the crop stage still
    writes the box; the outputs are the same and the statuses are the crop call's under the same flags"""
    import fpng_amd
    both = [(case, f) for f in VM.FILTERS for case in _cases(files, f)][1::3]
    cases, filters = [case for case, _ in both], [f for _, f in both]
    pngs = [files.pngs[k[0]] for k in cases]
    kinds = [KINDS[k % len(KINDS)] for k in range(len(cases))]
    try:
        enc.set_decode_verify(fpng_amd.VERIFY_CRC32 | fpng_amd.VERIFY_ADLER32)
        crops = [k[1] for k in cases]
        want = [st for st, _, _ in (enc.decode_device_crop(_device_files(pngs), crops) if device else enc.decode_batch_crop(pngs, crops))]
        assert want == [0] * len(cases)
        _run_cases(enc, files, model, cases, filters, 4, "bfloat16", device, [bool(k & 1) for k in range(len(cases))], kinds)
    finally:
        enc.set_decode_verify(0)


def test_a_descriptor_decodes_again_after_its_outputs_are_overwritten(enc, files, model):  # noqa: F811
    import torch
    cases = _cases(files, "bicubic")[::5]
    dev = _device_files([files.pngs[k[0]] for k in cases], shift=2)
    for dtype in ("uint8", "float32"):
        outs = [torch.zeros((3 + (k & 1),) + _window(full, window)[:1:-1], dtype=getattr(torch, dtype), device="cuda") for k, (_, _, full, window) in enumerate(cases)]
        kw = {} if dtype == "uint8" else {"scale": CONSTS[0][0], "bias": CONSTS[0][1]}
        db = enc.make_decode_batch_resize_view(dev, [k[1] for k in cases], outs, [k[2] for k in cases], [k[3] for k in cases], "bicubic",
                                               mirror=[bool(k & 2) for k in range(len(cases))], **kw)
        for again in range(2):
            for t in outs:
                t.fill_(1)
            assert enc.decode_device_resize_view(db, results=False) is db
            torch.cuda.synchronize()
            assert list(db.statuses()) == [0] * len(cases)
            for k, (case, t) in enumerate(zip(cases, outs)):
                bits = t.cpu().view(torch.uint8).numpy().view(BITS[ELEM[dtype]])
                want = _elements(model.view(*case, "bicubic"), 3 + (k & 1), dtype, bool(k & 2)).transpose(2, 0, 1)
                assert np.array_equal(bits, want), (dtype, again, k)
    with pytest.raises(ValueError):
        enc.decode_device_resize(db)  # (another call's descriptor)
    with pytest.raises(ValueError):
        enc.decode_batch_resize_view(db)  # (device files: decode_device_resize_view)
