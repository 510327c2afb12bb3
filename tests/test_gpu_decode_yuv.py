"""GPU decoder into YUV video surfaces (-m gpu; fpng_amd_decode_batch_yuv_views / fpng_amd_decode_batch_device_yuv_views: the planar
views path writes a view's three uint8 planes into the decode scratch, dec_yuv_store_kernel turns them into the caller's NV12,
P010 / P012 / P016 or planar 4:4:4 surface).

Expected values never come from the library: the pixels are the REFERENCE's decoder's (judge()), sliced to the view's crop, resized
and windowed by resize_view_model.py where the view resizes, and turned into the surface's elements by yuv_store_model.py.  Every
destination lies in a buffer prefilled with random bytes that is compared WHOLE: every element equal, nothing else written.

The shapes are the smallest at which the kernel can go wrong: a lane owns 8 pixels of a pair of rows, so widths of 1, 2, 3, 17, 63,
64, 65 (strips with 1 .. 8 pixels, odd last pairs), 513 (one strip past a wave's 64) and 1030 (a third workgroup along the row, a
strip of 6), heights that are odd, one pair, and past a workgroup's 4 pairs (33, 35)."""
import numpy as np
import pytest

import resize_view_model as VM
import yuv_store_model as SM
from test_gpu_decode import _device_files, enc, judge  # noqa: F401  (enc: a fixture)
from test_gpu_decode_layouts import _encode_gpu, _header_dims
from test_yuv_store_cpu import LAYOUTS, layout_of
from yuv_model import Layout

pytestmark = pytest.mark.gpu

CROP_OUTSIDE = 67
# (w, h, channels in the file, encode flags: 2 = stored)
IDENTITY = [(1, 1, 3, 0), (2, 2, 3, 0), (3, 5, 3, 0), (17, 9, 4, 0), (63, 33, 3, 0), (64, 16, 3, 2), (65, 17, 3, 1), (513, 3, 3, 0), (1030, 35, 3, 0)]


class _Files:
    """files written by the project's encoder, and the reference decoder's pixels of each as (3, h, w) planes (alpha dropped)"""

    def __init__(self, enc, specs):
        import fpng_amd
        rng = np.random.default_rng(17)
        self.dims, self.pngs, self.planes, self.imgs = [], [], [], []
        for n, (w, h, c, flags) in enumerate(specs):
            if n % 3 == 2:
                img = np.frombuffer(fpng_amd.synth_image("grad", w, h, c), dtype=np.uint8).reshape(h, w, c).copy()
                img[..., :3] ^= SM.content(rng, w, h) & 3  # (a gradient with noise in its low bits)
            else:
                img = np.concatenate([SM.content(rng, w, h), rng.integers(0, 256, (h, w, c - 3), dtype=np.uint8)], axis=2)
            (png,) = _encode_gpu(enc, [(img, flags)])
            st, px, pw, ph, pc = judge(png, 3)
            assert st == 0 and (pw, ph, pc) == (w, h, c)
            px = np.asarray(px).reshape(h, w, 3)
            assert np.array_equal(px, img[..., :3])
            self.dims.append((w, h)), self.pngs.append(png), self.imgs.append(img)
            self.planes.append(np.ascontiguousarray(px.transpose(2, 0, 1)))

    def view(self, i, crop=None, full=None, window=None, filter="bilinear", mirror=False):
        """the (oh, ow, 3) R,G,B bytes of a view of file i"""
        w, h = self.dims[i]
        x, y, cw, ch = crop if crop is not None else (0, 0, w, h)
        px = self.planes[i][:, y:y + ch, x:x + cw]
        full = full if full is not None else (cw, ch)
        if tuple(full) == (cw, ch) and window is None:  # (the identity)
            r = px[:, :, ::-1] if mirror else px
        else:
            r = VM.view_planes(px, full, window, filter, mirror)
        return np.ascontiguousarray(r.transpose(1, 2, 0))


@pytest.fixture(scope="module")
def identity_files(enc):  # noqa: F811
    return _Files(enc, IDENTITY)


@pytest.fixture(scope="module")
def some_files(enc):  # noqa: F811
    return _Files(enc, [(320, 200, 3, 0), (65, 17, 3, 0), (40, 24, 4, 0)])


class _Dest:
    """a surface inside a buffer of random bytes on the device"""

    def __init__(self, lay, rng):
        import torch
        self.lay = lay
        self.before = rng.integers(0, 256, lay.total, dtype=np.uint8)
        self.buf = torch.from_numpy(self.before.copy()).cuda()
        self.planes = lay.torch_views(self.buf)

    def expected(self, rgb, depth, m):
        exp = self.before.copy()
        SM.write(SM.surface(rgb, self.lay.surface, depth, m), self.lay.numpy_views(exp))
        return exp

    def check(self, exp, what):
        got = self.buf.cpu().numpy()
        if not np.array_equal(got, exp):
            at = int(np.flatnonzero(got != exp)[0])
            raise AssertionError((what, "first difference at byte", at, "of", got.size, "luma at", self.lay.luma, "pitch", self.lay.pitch, int(got[at]), int(exp[at])))

    def element_mask(self):
        m = np.zeros(self.lay.total, dtype=np.uint8)
        for v in self.lay.numpy_views(m):
            v[...] = np.array(-1).astype(v.dtype)
        return m != 0


def _sync():
    import torch
    torch.cuda.synchronize()


@pytest.mark.parametrize("surface,depth", SM.CASES)
def test_identity_views_of_every_size(enc, identity_files, surface, depth):  # noqa: F811
    """each file whole at its own size, all of them in one call: strips of every length, a 4-channel file (alpha dropped), a stored
    file and a 2-pass file among them"""
    f = identity_files
    rng = np.random.default_rng(23)
    m = SM.matrix("bt709", False)
    dests = [_Dest(Layout(surface, w, h), rng) for w, h in f.dims]
    got = enc.decode_device_yuv(_device_files(f.pngs, shift=1), [[d.planes] for d in dests], surface, depth, matrix=m)
    _sync()
    for i, ((st, views, cf), d) in enumerate(zip(got, dests)):
        assert st == 0 and cf == IDENTITY[i][2] and len(views) == 1, (i, st, cf)
        d.check(d.expected(f.view(i), depth, m), (surface, depth, f.dims[i]))


@pytest.mark.parametrize("surface,depth", SM.CASES)
def test_every_layout(enc, some_files, surface, depth):  # noqa: F811
    """the CPU test's layouts -- padded pitch, chroma far away, chroma in front of the luma, 8-bit planes at an odd byte, 16-bit
    planes at 2 mod 4 -- as six views of one 65 x 17 file in one call, in limited and full range"""
    f, i = some_files, 1
    w, h = f.dims[i]
    rng = np.random.default_rng(29)
    for full_range in (False, True):
        m = SM.matrix("bt601", full_range)
        dests = [_Dest(layout_of(surface, w, h, kw), rng) for kw in LAYOUTS]
        got = enc.decode_device_yuv(_device_files([f.pngs[i]]), [[d.planes for d in dests]], surface, depth, crops=[[(0, 0, w, h)] * len(dests)], standard="bt601",
                                    full_range=full_range)
        _sync()
        assert got[0][0] == 0 and len(got[0][1]) == len(dests)
        exp_rgb = f.view(i)
        for kw, d in zip(LAYOUTS, dests):
            d.check(d.expected(exp_rgb, depth, m), (surface, depth, kw, full_range))


@pytest.mark.parametrize("surface,depth", [("nv12", 8), ("p016", 10), ("yuv444", 8), ("yuv444_16", 16)])
def test_resize_window_and_mirror_in_one_call(enc, some_files, surface, depth):  # noqa: F811
    """one 320 x 200 file into 160 x 90 bilinear, 107 x 61 bicubic mirrored, and a 64 x 48 window at (5, 3) of a 150 x 100 resize"""
    f, i = some_files, 0
    rng = np.random.default_rng(31)
    m = SM.matrix("bt709", False)
    whole = (0, 0, 320, 200)
    views = [(whole, (160, 90), None, "bilinear", False), ((3, 2, 300, 190), (107, 61), None, "bicubic", True), (whole, (150, 100), (5, 3, 64, 48), "bilinear", False)]
    sizes = [(160, 90), (107, 61), (64, 48)]
    dests = [_Dest(Layout(surface, ow, oh, pitch_pad=2 * SM.elem_bytes(surface) * (k & 1)), rng) for k, (ow, oh) in enumerate(sizes)]
    got = enc.decode_device_yuv(_device_files([f.pngs[i]], shift=2), [[d.planes for d in dests]], surface, depth, crops=[[v[0] for v in views]], full=[[v[1] for v in views]],
                                window=[[v[2] for v in views]], filter=[[v[3] for v in views]], mirror=[[v[4] for v in views]])
    _sync()
    assert got[0][0] == 0
    for v, d in zip(views, dests):
        d.check(d.expected(f.view(i, *v), depth, m), (surface, depth, v))


def test_a_batch_with_a_crop_outside_and_a_damaged_file(enc, some_files):  # noqa: F811
    """three files of different sizes in one batch: one whose crop leaves the image (status 67, its surface untouched), one damaged by
    token_mutator -- its status is the planar views call's for the same input, and nothing outside its elements is written"""
    from test_decode_model import edited_files
    f = some_files
    rng = np.random.default_rng(37)
    m = SM.matrix("bt2020", False)
    cands = [(png, _header_dims(png)) for _, png in edited_files(np.random.default_rng(5), 6)]
    cands = [(png, d) for png, d in cands if d != (1, 1) and d[0] * d[1] <= 1 << 16]
    assert cands
    crops = [[(0, 0, w, h)] for _, (w, h) in cands]
    planar = enc.decode_device_views(_device_files([p for p, _ in cands]), crops, None, [[(w, h)] for _, (w, h) in cands])
    _sync()
    bad = [k for k, (st, _, _) in enumerate(planar) if st != 0]
    assert bad, "no damaged file among the candidates"
    for surface, depth in (("nv12", 8), ("p016", 12)):
        # every candidate: the same status as the planar views call
        ds = [_Dest(Layout(surface, w, h), rng) for _, (w, h) in cands]
        got = enc.decode_device_yuv(_device_files([p for p, _ in cands]), [[d.planes] for d in ds], surface, depth, crops=crops, matrix=m)
        _sync()
        assert [st for st, _, _ in got] == [st for st, _, _ in planar]
        for d in ds:
            keep = ~d.element_mask()
            assert np.array_equal(d.buf.cpu().numpy()[keep], d.before[keep])
        # the batch of three
        k = bad[0]
        pngs = [f.pngs[0], cands[k][0], f.pngs[2]]
        dims = [f.dims[0], cands[k][1], f.dims[2]]
        crops3 = [[(0, 0) + dims[0]], [(0, 0) + dims[1]], [(8, 8, 40, 24)]]  # (file 2 is 40 x 24: the crop leaves it)
        dests = [_Dest(Layout(surface, w, h, pitch_pad=2), rng) for w, h in (dims[0], dims[1], (40, 24))]
        got = enc.decode_device_yuv(_device_files(pngs, shift=3), [[d.planes] for d in dests], surface, depth, crops=crops3, matrix=m)
        _sync()
        assert [st for st, _, _ in got] == [0, planar[k][0], CROP_OUTSIDE] and got[1][1] is None and got[2][1] is None
        dests[0].check(dests[0].expected(f.view(0), depth, m), (surface, "file 0"))
        keep = ~dests[1].element_mask()
        assert np.array_equal(dests[1].buf.cpu().numpy()[keep], dests[1].before[keep])
        dests[2].check(dests[2].before, (surface, "the crop-outside file's surface is unchanged"))


@pytest.mark.parametrize("surface,depth", SM.CASES)
def test_equals_the_planar_views_call_through_the_host_twin(enc, some_files, surface, depth):  # noqa: F811
    """the same file, crop and view through decode_device_views into uint8 planes, then fpng_amd_yuv_surface on the host: the
    surfaces of decode_device_yuv, allocated tight by the call, are equal"""
    import fpng_amd
    f, i = some_files, 0
    crops, fulls, windows = [[(10, 6, 301, 187), (0, 0, 320, 200)]], [[(97, 55), (320, 200)]], [[(1, 2, 95, 51), None]]
    kw = dict(filter=[["bicubic", "bilinear"]], mirror=[[True, False]])
    planar = enc.decode_device_views(_device_files([f.pngs[i]]), crops, None, fulls, windows, **kw)
    got = enc.decode_device_yuv(_device_files([f.pngs[i]]), None, surface, depth, crops=crops, full=fulls, window=windows, standard="bt2020", full_range=True, **kw)
    _sync()
    assert planar[0][0] == 0 and got[0][0] == 0 and len(got[0][1]) == 2
    for t, planes in zip(planar[0][1], got[0][1]):
        rgb = np.ascontiguousarray(t.cpu().numpy().transpose(1, 2, 0))
        want = fpng_amd.yuv_surface(rgb, surface, depth, standard="bt2020", full_range=True)
        assert len(planes) == len(want)
        for a, b in zip(planes, want):
            a = a.cpu().numpy()
            assert a.shape == b.shape and np.array_equal(a.view(b.dtype), b)


@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("standard,full_range", [("bt601", False), ("bt709", True), ("bt2020", False)])
def test_round_trip_through_the_encoder(enc, flags, standard, full_range):  # noqa: F811
    """a 3-channel file -> yuv444_16 at depth 16 -> Encoder.encode_yuv with yuv_matrix of the same standard and range: the file,
    byte for byte, at the same flags"""
    rng = np.random.default_rng(41)
    img = SM.content(rng, 97, 41)
    (png,) = _encode_gpu(enc, [(img, flags)])
    got = enc.decode_device_yuv(_device_files([png]), None, "yuv444_16", 16, standard=standard, full_range=full_range)
    assert got[0][0] == 0
    (again,) = enc.encode_yuv([got[0][1][0]], surface="yuv444_16", standard=standard, full_range=full_range, flags=flags)
    assert bytes(again) == bytes(png)


def test_host_files(enc, identity_files):  # noqa: F811
    """one host-resident batch through decode_batch_yuv: every file of the identity set and two views of the last"""
    f = identity_files
    rng = np.random.default_rng(43)
    m = SM.matrix("bt709", False)
    last = len(f.pngs) - 1
    w, h = f.dims[last]
    dests = [[_Dest(Layout("nv12", w_, h_, place="far"), rng)] for w_, h_ in f.dims]
    dests[last].append(_Dest(Layout("nv12", 200, 20), rng))
    crops = [[(0, 0, w_, h_)] for w_, h_ in f.dims]
    crops[last].append((0, 0, w, h))
    fulls = [[(w_, h_)] for w_, h_ in f.dims]
    fulls[last].append((200, 20))
    got = enc.decode_batch_yuv([bytes(p) for p in f.pngs], [[d.planes for d in ds] for ds in dests], "nv12", crops=crops, full=fulls, matrix=m)
    _sync()
    for i, ((st, views, _), ds) in enumerate(zip(got, dests)):
        assert st == 0 and len(views) == len(ds), (i, st)
        ds[0].check(ds[0].expected(f.view(i), 8, m), ("host", f.dims[i]))
    dests[last][1].check(dests[last][1].expected(f.view(last, (0, 0, w, h), (200, 20)), 8, m), "host, the resized view")
