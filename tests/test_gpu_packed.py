"""GPU tests (-m gpu) of packed submissions (fpng_amd_encode_submit_packed): a submission's files back to back in one arena, placed
on the GPU from their actual sizes.  The bar for the files is the reference (test_gpu_layouts._expect: cpu_ref.ref() or the pinned
oracle), for the placement fpng_amd_pack_place (judged against a model in test_packed_cpu.py), and for everything else the arena's
prefill: a byte outside the placed files' extents that does not hold the pattern any more was written."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_layouts import _content, _expect, _fmt, _layout, _same, _to_source

pytestmark = pytest.mark.gpu

INVALID_ARG, ARENA_FULL = -1, 2
SHAPES = [(1, 1), (63, 5), (64, 3), (257, 4), (1000, 17), (7680, 4)]  # (w, h)
PLACINGS = [(16, 0), (64, 16), (512, 512)]  # (align, lead)


@pytest.fixture(scope="module")
def enc(built_lib):
    import torch
    import fpng_amd
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    e = fpng_amd.Encoder(device=0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def contents():
    return {(w, h, c): _content(i, w, h, c) for i, (w, h) in enumerate(SHAPES) for c in (3, 4)}


@pytest.fixture(scope="module")
def expected():
    """the judge's file for (pixels, flags), made once per distinct image"""
    made = {}

    def get(img, flags):
        key = (img.shape, img.tobytes(), flags)
        if key not in made:
            made[key] = _expect(img, flags)
        return made[key]
    return get


def _up(v, a):
    return -(-v // a) * a


def _pattern(n):
    return (np.arange(n, dtype=np.uint32) * 7 % 251 + 1).astype(np.uint8)  # never zero


def _arena(nbytes, align):
    """-> (arena: a CUDA uint8 view of nbytes + 4096 bytes whose address is a multiple of align, prefilled; the prefill on the host).
    Tests hand the encoder arena[:cap]: the bytes behind it are watched as well."""
    import torch
    raw = torch.empty(nbytes + 4096 + align, dtype=torch.uint8, device="cuda")
    skip = (-raw.data_ptr()) % align
    arena = raw[skip:skip + nbytes + 4096]
    pat = _pattern(arena.numel())
    arena.copy_(torch.from_numpy(pat))
    return arena, pat


def _need(sizes, align, lead, k=None):
    """bytes the first k files need (the cursor behind them), by the rule"""
    import fpng_amd
    k = len(sizes) if k is None else k
    if k == 0:
        return 0
    recs, _ = fpng_amd.pack_place(sizes[:k], align, lead, 1 << 62)
    return recs[-1][0] + _up(sizes[k - 1], 16)


def _check(arena, pat, recs, total, want_files, sizes, align, lead, cap, what):
    """recs as wait_packed() gives them, against the rule on `sizes` (the reference's) and the reference's files; the arena outside
    the placed extents against the prefill"""
    import fpng_amd
    want, want_total = fpng_amd.pack_place(sizes, align, lead, cap)
    host = arena.cpu().numpy()
    untouched = np.ones(host.size, dtype=bool)
    for i, ((off, size, mode, status), (w_off, w_st), png) in enumerate(zip(recs, want, want_files)):
        assert (off, status) == (w_off, w_st), f"{what}: file {i} at {off} status {status}, the rule says {w_off} / {w_st}"
        if status:
            assert size == 0 and off == 0, f"{what}: refused file {i} reports size {size} offset {off}"
            continue
        assert off % 16 == 0 and (off - lead) % align == 0 and off + _up(size, 16) <= cap
        _same(bytes(host[off:off + size]), png, f"{what}: file {i}")
        untouched[off:off + _up(size, 16)] = False
    assert total == want_total, f"{what}: total {total}, the rule says {want_total}"
    bad = np.flatnonzero(untouched & (host != pat))
    assert not bad.size, f"{what}: {bad.size} arena bytes outside the placed files were written, the first at {int(bad[0])} (cap {cap})"


def _tensors(imgs):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(im)).cuda() for im in imgs]


def _run(enc, imgs, flags, align, lead, expected, what, cap=None, with_table=True):
    """one packed submission of HWC images through the Python door, everything checked; -> records"""
    import torch
    import fpng_amd
    files = [expected(im, flags) for im in imgs]
    sizes = [len(f) for f in files]
    full = fpng_amd.pack_capacity([(im.shape[1], im.shape[0], im.shape[2]) for im in imgs], align, lead)
    cap = full if cap is None else cap
    arena, pat = _arena(max(full, cap), align)
    n = len(imgs)
    table = torch.full((2 * (n + 1),), -1, dtype=torch.int64, device="cuda") if with_table else None
    assert enc.submit_packed(_tensors(imgs), arena[:cap], align=align, lead=lead, table=table, flags=flags) == n
    recs, total = enc.wait_packed(enc.last_ticket, n)
    _check(arena, pat, recs, total, files, sizes, align, lead, cap, what)
    if with_table:
        t = table.cpu().numpy().reshape(n + 1, 2)
        assert [tuple(r) for r in t[:n]] == [(off, size) for off, size, _, _ in recs], f"{what}: d_table differs from the host records"
        assert tuple(t[n]) == (total, sum(1 for r in recs if not r[3])), f"{what}: d_table's last pair"
    return recs


@pytest.mark.parametrize("placing", PLACINGS)
@pytest.mark.parametrize("flags", [0, 1, 2])
def test_parity_and_placement(enc, contents, expected, flags, placing):
    align, lead = placing
    imgs = [contents[(w, h, c)] for (w, h) in SHAPES for c in (3, 4)]
    recs = _run(enc, imgs, flags, align, lead, expected, f"flags {flags} align {align} lead {lead}")
    assert all(st == 0 for _, _, _, st in recs)
    if flags == 2:
        assert all(mode == 1 for _, _, mode, _ in recs)


def test_stored_fallback_inside_a_batch(enc, contents, expected):
    """noise (the device decides for stored blocks, and only then is the size known) between compressible images"""
    import fpng_amd
    noise = [fpng_amd.synth_image("noise", w, h, c, seed=5 + w) for (w, h, c) in [(300, 40, 3), (64, 3, 4), (1000, 17, 4)]]
    imgs = [contents[(1000, 17, 3)], noise[0], contents[(257, 4, 4)], noise[1], noise[2], contents[(63, 5, 3)]]
    for align, lead in [(16, 0), (512, 512)]:
        recs = _run(enc, imgs, 0, align, lead, expected, f"stored inside a batch, align {align}")
        assert [mode for _, _, mode, _ in recs] == [0, 1, 0, 1, 1, 0]


@pytest.mark.parametrize("flags", [0, 1])
def test_arena_full(enc, contents, expected, flags):
    imgs = [contents[k] for k in [(1000, 17, 3), (63, 5, 4), (257, 4, 3), (64, 3, 3), (1000, 17, 4), (1, 1, 4)]]
    sizes = [len(expected(im, flags)) for im in imgs]
    n = len(imgs)
    for align, lead in [(16, 0), (512, 512)]:
        need = _need(sizes, align, lead)
        caps = [(need, 0), (need - 1, 1), (16, n)] + [(_need(sizes, align, lead, k), n - k) for k in (4, 1)]
        for cap, refused in caps:
            recs = _run(enc, imgs, flags, align, lead, expected, f"arena of {cap} (need {need}) align {align} flags {flags}", cap=cap)
            assert [st for _, _, _, st in recs] == [0] * (n - refused) + [ARENA_FULL] * refused
    # a file refused before placement cannot be made at these sizes (it takes a stored file past 4 GiB); what the rule
    # does with one is test_packed_cpu.py's


@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("n", [1, 2, 64, 65, 256, 257, 1025])
def test_job_counts_around_the_placement_kernels_widths(enc, expected, n, flags):
    """one wave, one round of 256, a second round with a carry, five rounds; n = 1 is the submission whose record travels in the
    kernel arguments"""
    base = [_content(40 + i, w, h, c) for i, (w, h, c) in enumerate([(4, 4, 3), (5, 3, 4), (4, 4, 4), (5, 3, 3), (4, 4, 3)])]
    imgs = [base[(i * 3 + i // 5) % 5] for i in range(n)]
    _run(enc, imgs, flags, 64, 16, expected, f"n {n} flags {flags}")


def _submit_raw(enc, kind, arr, n, fmt, flags, pack):
    t = C.c_uint64(0)
    enc._sync_stream()
    rc = enc.lib.fpng_amd_encode_submit_packed(enc.h, kind, C.cast(arr, C.c_void_p) if arr is not None else None, n,
                                               C.byref(fmt) if fmt is not None else None, flags, C.byref(pack) if pack is not None else None, C.byref(t))
    return rc, t.value


def _pack(arena, cap, align=16, lead=0, table=None, reserved=0):
    from fpng_amd import _lib
    return _lib.Pack(arena.data_ptr(), cap, align, lead, table, reserved)


@pytest.mark.parametrize("flags", [0, 1, 2])
def test_all_four_descriptor_kinds(enc, contents, expected, flags):
    """each kind once, in a layout of its own test file -- an ex BGRA crop with a negative pitch, planes in reverse order, f16 planes
    with mean / std -- with that file's expectation: the reference on the pixels as R,G,B[,A]; the last file of every submission
    finds no room, so that every kind's way past a refused file runs too"""
    import torch
    from fpng_amd import _lib
    import test_gpu_float_encode as tf
    import test_gpu_planar as tp
    from test_float_encode_cpu import float_image
    a, b = contents[(257, 4, 4)], contents[(1000, 17, 3)]
    a3 = contents[(257, 4, 3)]
    keep = []

    def ex_descs():
        arr = (_lib.ImageEx * 3)()
        for d, (img, name) in zip(arr, [(a, "BGRA"), (b, "BGR"), (a, "BGRA")]):
            buf, top, pitch = _layout(_to_source(img, name, None), "neg", np.random.default_rng(3))
            dev = torch.from_numpy(buf).cuda()
            keep.append(dev)
            d.d_pixels, d.row_pitch, d.w, d.h, d.format = dev.data_ptr() + top, pitch, img.shape[1], img.shape[0], _fmt(name)[0]
        return arr, [a, b, a], None

    def planar_descs():
        arr = (_lib.ImagePlanar * 3)()
        for d, img in zip(arr, [a, b, a3]):
            buf, top, rp, pp = tp._planes(img, "rev", np.random.default_rng(4))
            dev = torch.from_numpy(buf).cuda()
            keep.append(dev)
            d.d_pixels, d.row_pitch, d.plane_pitch, (d.h, d.w, d.num_chans) = dev.data_ptr() + top, rp, pp, img.shape
        return arr, [a, b, a3], None

    def float_descs():
        to_float, scale, bias = tf.VARIANTS["meanstd"]
        arr, imgs = (_lib.ImagePlanar * 3)(), []
        for d, img in zip(arr, [a, b, a3]):
            el, by = float_image(img, 1, scale, bias, np.random.default_rng(5), to_float)
            buf, top, rp, pp = tf._planes(el, 1, "rev", np.random.default_rng(6))
            dev = torch.from_numpy(buf.view(np.uint8)).cuda()
            keep.append(dev)
            d.d_pixels, d.row_pitch, d.plane_pitch, (d.h, d.w, d.num_chans) = dev.data_ptr() + 2 * top, 2 * rp, 2 * pp, el.shape
            imgs.append(by)
        fmt = _lib.FloatFormat()
        fmt.dtype = 1
        for k in range(4):
            fmt.scale[k], fmt.bias[k] = float(scale[k]), float(bias[k])
        return arr, imgs, fmt

    def image_descs():
        arr = (_lib.Image * 3)()
        for d, img in zip(arr, [a, b, a3]):
            dev = torch.from_numpy(img).cuda()
            keep.append(dev)
            d.d_pixels, (d.h, d.w, d.num_chans) = dev.data_ptr(), img.shape
        return arr, [a, b, a3], None

    for kind, make in [(_lib.DESC_IMAGE, image_descs), (_lib.DESC_EX, ex_descs), (_lib.DESC_PLANAR, planar_descs), (_lib.DESC_PLANAR_FLOAT, float_descs)]:
        arr, imgs, fmt = make()
        files = [expected(np.ascontiguousarray(im), flags) for im in imgs]
        sizes = [len(f) for f in files]
        cap = _need(sizes, 64, 16, 2)
        arena, pat = _arena(_need(sizes, 64, 16), 64)
        rc, t = _submit_raw(enc, kind, arr, 3, fmt, flags, _pack(arena, cap, 64, 16))
        assert rc == 0, enc.lib.fpng_amd_last_error()
        recs, total = enc.wait_packed(t, 3)
        assert [st for _, _, _, st in recs] == [0, 0, ARENA_FULL]
        _check(arena, pat, recs, total, files, sizes, 64, 16, cap, f"kind {kind} flags {flags}")


@pytest.mark.parametrize("flags", [0, 1, 2])
def test_single_job_submissions_of_every_kind(enc, contents, expected, flags):
    """n = 1 through every submit method, one after the other: the plain kind's record travels in the kernel arguments, every other
    kind's is uploaded, and each kind has kernels of its own -- every file is the reference's for the pixels, and the tickets are
    consecutive.  The rendition is the whole image at its own size, so its pixels are the source's."""
    import torch
    import fpng_amd
    tickets = []
    for img in (contents[(63, 5, 3)], _content(7, 16, 3, 4)):
        h, w, c = img.shape
        want = expected(img, flags)
        dev = torch.from_numpy(img).cuda()
        swapped = dev[..., [2, 1, 0, 3][:c]].contiguous()  # B,G,R[,A]
        chw = dev.permute(2, 0, 1).contiguous()
        as_float = chw.to(torch.float32) / 255.0  # (rint(fl(b / 255) * 255) is b)
        arena, _ = _arena(fpng_amd.pack_capacity([(w, h, c)]), 16)
        doors = [("submit", lambda o: enc.submit([dev], [o], flags)),
                 ("submit_ex", lambda o: enc.submit_ex([swapped], [o], flags, order="bgr")),
                 ("submit_planar", lambda o: enc.submit_planar([chw], [o], flags)),
                 ("submit_float", lambda o: enc.submit_float([as_float], [o], flags)),
                 ("submit_packed", lambda o: enc.submit_packed([dev], arena[:arena.numel() - 4096], flags=flags)),
                 ("submit_renditions", lambda o: enc.submit_renditions([dev], [fpng_amd.rendition(0, (w, h))], outs=[o], flags=flags))]
        for name, door in doors:
            out = torch.zeros(fpng_amd.max_encoded_size(w, h, c) + 64, dtype=torch.uint8, device="cuda")
            assert door(out) == 1
            tickets.append(enc.last_ticket)
            if name == "submit_packed":
                ((off, size, mode, status),), _ = enc.wait_packed(enc.last_ticket, 1)
                out = arena[off:]
            else:
                ((size, mode, status),) = enc.wait(enc.last_ticket, 1)
            assert status == 0 and mode == (1 if flags == 2 else mode), (name, status, mode)
            _same(bytes(out[:size].cpu().numpy()), want, f"{name}, n = 1, {w} x {h} x {c}, flags {flags}")
    assert tickets == list(range(tickets[0], tickets[0] + len(tickets))), tickets


def test_ordering(enc, contents, expected):
    import torch
    import fpng_amd
    imgs = [contents[k] for k in [(1000, 17, 3), (257, 4, 4), (63, 5, 3)]]
    files = [expected(im, 0) for im in imgs]
    sizes = [len(f) for f in files]
    dims = [(im.shape[1], im.shape[0], im.shape[2]) for im in imgs]
    dev = _tensors(imgs)
    # a packed submission between a plain and a planar one, none waited for in between
    outs = [torch.empty(fpng_amd.max_encoded_size(*d) + 64, dtype=torch.uint8, device="cuda") for d in dims]
    outs_pl = [torch.empty_like(o) for o in outs]
    chw = [t.permute(2, 0, 1).contiguous() for t in dev]
    arena, pat = _arena(fpng_amd.pack_capacity(dims, 64, 16), 64)
    cap = arena.numel() - 4096
    enc.submit(dev, outs, 0)
    t_plain = enc.last_ticket
    enc.submit_packed(dev, arena[:cap], align=64, lead=16)
    t_packed = enc.last_ticket
    enc.submit_planar(chw, outs_pl, 0)
    t_planar = enc.last_ticket
    assert t_packed == t_plain + 1 and t_planar == t_packed + 1
    for res, bufs in [(enc.wait(t_planar, 3), outs_pl), (enc.wait(t_plain, 3), outs)]:
        for (size, _, status), out, f in zip(res, bufs, files):
            assert status == 0
            _same(bytes(out[:size].cpu().numpy()), f, "a neighbour of the packed submission")
    # wait() on a packed ticket: the sizes, without offsets; wait_packed() on a plain one is refused
    assert [(s, st) for s, _, st in enc.wait(t_packed, 3)] == [(s, 0) for s in sizes]
    recs, total = enc.wait_packed(t_packed, 3)
    _check(arena, pat, recs, total, files, sizes, 64, 16, cap, "between a plain and a planar submission")
    with pytest.raises(fpng_amd.FpngAmdError) as err:
        enc.wait_packed(t_plain, 3)
    assert err.value.code == INVALID_ARG
    # two packed submissions in flight into two arenas
    a1, p1 = _arena(fpng_amd.pack_capacity(dims, 16, 0), 16)
    a2, p2 = _arena(fpng_amd.pack_capacity(dims[::-1], 512, 512), 512)
    enc.submit_packed(dev, a1[:a1.numel() - 4096])
    t1 = enc.last_ticket
    enc.submit_packed(dev[::-1], a2[:a2.numel() - 4096], align=512, lead=512, flags=1)
    t2 = enc.last_ticket
    r2, tot2 = enc.wait_packed(t2, 3)
    r1, tot1 = enc.wait_packed(t1, 3)
    _check(a1, p1, r1, tot1, files, sizes, 16, 0, a1.numel() - 4096, "first of two in flight")
    files2 = [expected(im, 1) for im in imgs[::-1]]
    _check(a2, p2, r2, tot2, files2, [len(f) for f in files2], 512, 512, a2.numel() - 4096, "second of two in flight")
    # a torch producer on the current stream in front, a torch consumer behind join(): no host wait in between
    a3, p3 = _arena(fpng_amd.pack_capacity(dims, 64, 16), 64)
    table = torch.full((8,), -1, dtype=torch.int64, device="cuda")
    big = torch.zeros(1 << 24, dtype=torch.uint8, device="cuda")
    for _ in range(4):
        big.add_(1)  # (something for the stream to be busy with)
    produced = [((t.to(torch.int16) + 3) & 255).to(torch.uint8) for t in dev]
    enc.submit_packed(produced, a3[:a3.numel() - 4096], align=64, lead=16, table=table)
    t3 = enc.last_ticket
    enc.join()
    seen, seen_table = a3.clone(), table.clone()  # on torch's stream, behind the join
    host, tab = seen.cpu().numpy(), seen_table.cpu().numpy().reshape(4, 2)
    files3 = [expected(((im.astype(np.int16) + 3) & 255).astype(np.uint8), 0) for im in imgs]
    assert tab[3][1] == 3
    for (off, size), f in zip(tab[:3], files3):
        _same(bytes(host[off:off + size]), f, "read behind join() from the device table")
    r3, tot3 = enc.wait_packed(t3, 3)
    assert [(o, s) for o, s, _, _ in r3] == [tuple(r) for r in tab[:3]] and tot3 == tab[3][0]
    _check(a3, p3, r3, tot3, files3, [len(f) for f in files3], 64, 16, a3.numel() - 4096, "torch producer")


def test_validation(enc, contents, expected):
    """every refusal: its code, no ticket, the arena untouched -- and the next valid submission works and gets the next ticket"""
    import torch
    from fpng_amd import _lib
    img = contents[(63, 5, 3)]
    dev = torch.from_numpy(img).cuda()
    arena, pat = _arena(4096, 512)
    table = torch.zeros(8, dtype=torch.int64, device="cuda")
    other = torch.zeros(4096, dtype=torch.uint8, device="cuda")

    def image(**kw):
        arr = (_lib.Image * 1)()
        arr[0].d_pixels, arr[0].w, arr[0].h, arr[0].num_chans = dev.data_ptr(), 63, 5, 3
        for k, v in kw.items():
            setattr(arr[0], k, v)
        return arr

    planar = (_lib.ImagePlanar * 1)()
    planar[0].d_pixels, planar[0].w, planar[0].h, planar[0].num_chans = dev.data_ptr(), 21, 5, 3
    fmt = _lib.FloatFormat()
    fmt.scale[:] = [255.0] * 4
    ok = dict(kind=0, arr=image(), fmt=None, pack=_pack(arena, 4096, 512, 512, table.data_ptr()))
    rc, t0 = _submit_raw(enc, ok["kind"], ok["arr"], 1, None, 0, ok["pack"])
    assert rc == 0
    enc.wait_packed(t0, 1)
    arena.copy_(torch.from_numpy(pat))
    bad = [
        ("unknown kind", dict(kind=4)),
        ("null pack", dict(pack=None)),
        ("null arena", dict(pack=_lib.Pack(None, 4096, 16, 0, None, 0))),
        ("align 24", dict(pack=_pack(arena, 4096, 24))), ("align 8", dict(pack=_pack(arena, 4096, 8))),
        ("align 131072", dict(pack=_pack(arena, 4096, 131072))),
        ("lead 8", dict(pack=_pack(arena, 4096, 16, 8))), ("lead too large", dict(pack=_pack(arena, 4096, 16, 65552))),
        ("arena not aligned", dict(pack=_pack(arena[16:], 4000, 512))), ("arena odd", dict(pack=_pack(arena[8:], 4000, 16))),
        ("table misaligned", dict(pack=_pack(arena, 4096, 16, 0, table.data_ptr() + 4))),
        ("reserved", dict(pack=_pack(arena, 4096, 16, 0, None, 1))),
        ("d_out given", dict(arr=image(d_out=other.data_ptr()))), ("out_cap given", dict(arr=image(out_cap=4096))),
        ("fmt for a plain kind", dict(fmt=fmt)), ("fmt for planar", dict(kind=2, arr=planar, fmt=fmt)),
        ("no fmt for float", dict(kind=3, arr=planar)),
        ("null images", dict(arr=None)),
        # the kinds' own source checks hold unchanged
        ("w = 0", dict(arr=image(w=0))), ("null pixels", dict(arr=image(d_pixels=None))), ("five channels", dict(arr=image(num_chans=5))),
    ]
    for what, kw in bad:
        args = dict(ok, **kw)
        rc, t = _submit_raw(enc, args["kind"], args["arr"], 1, args["fmt"], 0, args["pack"])
        assert rc == INVALID_ARG and t == 0, (what, rc, t, enc.lib.fpng_amd_last_error())
    torch.cuda.synchronize()
    assert np.array_equal(arena.cpu().numpy(), pat) and not other.any(), "a refused submission wrote something"
    rc, t1 = _submit_raw(enc, ok["kind"], ok["arr"], 1, None, 0, ok["pack"])
    assert rc == 0 and t1 == t0 + 1, "a refused submission took a ticket"
    recs, total = enc.wait_packed(t1, 1)
    f = expected(img, 0)
    _check(arena, pat, recs, total, [f], [len(f)], 512, 512, 4096, "after the refusals")
    # more records than images
    res = (_lib.PackedResult * 2)()
    assert enc.lib.fpng_amd_encode_wait_packed(enc.h, t1, res, 2, None) == INVALID_ARG


def test_round_trip_with_the_decoder(enc, contents, expected):
    """the decoder takes device files at any address: the views arena[off:off + size] decode to the source pixels"""
    import torch
    import fpng_amd
    imgs = [contents[k] for k in [(1000, 17, 4), (63, 5, 4), (7680, 4, 4), (257, 4, 4)]]
    for flags, (align, lead) in [(0, (16, 0)), (1, (64, 16)), (2, (512, 512))]:
        arena, recs = enc.encode_packed(_tensors(imgs), align=align, lead=lead, flags=flags)
        assert arena.data_ptr() % align == 0 and all(st == 0 for _, _, _, st in recs)
        views = [arena[off:off + size] for off, size, _, _ in recs]
        assert recs[-1][0] + recs[-1][1] == arena.numel()
        outs = [torch.zeros(im.shape, dtype=torch.uint8, device="cuda") for im in imgs]
        for (st, view, chans), im in zip(enc.decode_device_ex(views, outs, order="rgb"), imgs):
            assert st == 0 and chans == 4 and np.array_equal(view.cpu().numpy(), im)
