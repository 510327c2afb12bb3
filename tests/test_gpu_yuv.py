"""GPU tests (-m gpu) of fpng_amd_encode_submit_yuv: video frames in NV12, P016, planar 4:4:4 and 16-bit planar 4:4:4, converted inside
the row walk and encoded as 3-channel files.  The bar for the pixels is yuv_model.to_rgb (numpy, exact fp32), for the files
test_gpu_layouts._expect (the reference, or the pinned oracle) of those pixels, byte for byte, in flags 0, 1 and 2; for a packed
call's placement fpng_amd.pack_place on the judge's sizes; for renditions the files submit_renditions(kind="image") writes for the
model's RGB frame.  Nothing expected comes from the new code."""
import numpy as np
import pytest

import yuv_model as ym
from test_gpu_layouts import _expect, _same
from test_gpu_packed import _arena, _check, _need

pytestmark = pytest.mark.gpu

FLAGS = [0, 1, 2]
# odd widths and heights, the 64-pixel window edges, the 256-pixel super-window edges, several chroma rows
SIZES = [(1, 1), (1, 2), (2, 1), (3, 3), (63, 5), (64, 3), (65, 4), (255, 3), (256, 2), (257, 3), (1001, 7), (3840, 2)]
# (pitch_pad in bytes, place, start in elements): tight; pitch + 256 bytes; the chroma far away; in front of the luma; 8-bit planes at
# an odd byte / 16-bit planes at 2 mod 4
LAYOUTS = [(0, "tight", 0), (256, "tight", 0), (0, "far", 0), (0, "front", 0), (0, "far", 1)]
MATRICES = [("bt709", False), ("bt601", True), ("bt2020", False)]


@pytest.fixture(scope="module")
def enc(built_lib):
    import torch
    import fpng_amd
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    e = fpng_amd.Encoder(device=0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def expected():
    """the judge's file for (pixels, flags), made once per distinct image"""
    made = {}

    def get(img, flags):
        key = (img.shape, img.tobytes(), flags)
        if key not in made:
            made[key] = _expect(np.ascontiguousarray(img), flags)
        return made[key]
    return get


def _paint(planes, kind, rng):
    """content of the planes (the buffer around them stays random): 0 = noise over the whole element range; 1 = runs of equal
    elements, rows repeated in pairs (runs of equal PIXELS, rows equal to the row above: the walk's run tiers and zero rows);
    2 = a slope with a few spikes (short runs between literals)"""
    if kind == 0:
        return
    top = 1 << (8 * planes[0].dtype.itemsize)
    for p in planes:
        rows, cols = p.shape[0], p.shape[1]
        tail = p.shape[2:]
        if kind == 1:
            v = rng.integers(0, top, (-(-rows // 2), -(-cols // 24)) + tail)
            v = np.repeat(np.repeat(v, 2, axis=0), 24, axis=1)[:rows, :cols]
        else:
            v = (np.arange(cols).reshape((1, cols) + (1,) * len(tail)) * (top // 4096 + 1) // 8 * 8 + np.arange(rows).reshape((rows, 1) + (1,) * len(tail)) * 3) % top
            v = np.broadcast_to(v, p.shape).copy()
            spikes = rng.random(p.shape) < 0.02
            v[spikes] = rng.integers(0, top, int(spikes.sum()))
        p[...] = v.astype(p.dtype)


def _case(surface, w, h, layout, seed, content):
    """-> (Layout, the host buffer, the model's RGB pixels under MATRICES[seed % 3], the matrix)"""
    rng = np.random.default_rng(seed)
    e = ym.elem_bytes(surface)
    pad, place, start = layout
    lay = ym.Layout(surface, w, h, pitch_pad=pad, place=place, start=start * e)
    buf, planes = ym.fill_surface(lay, rng, "msb10" if (e == 2 and seed % 4 == 3 and content == 0) else "full")
    _paint(planes, content, rng)
    m = ym.matrix(*MATRICES[seed % 3])
    return lay, buf, np.ascontiguousarray(ym.to_rgb(surface, planes, m)), m


@pytest.fixture(scope="module")
def sweep():
    """per surface, per matrix: [(Layout, buffer, rgb)] over SIZES, the layouts and contents taking turns -- built once, shared by
    the flags"""
    out = {}
    for si, surface in enumerate(ym.SURFACES):
        groups = {}
        for i, (w, h) in enumerate(SIZES):
            lay, buf, rgb, _ = _case(surface, w, h, LAYOUTS[(i + si) % len(LAYOUTS)], 100 * si + i, (i // 2 + si) % 3)
            groups.setdefault((100 * si + i) % 3, []).append((lay, buf, rgb))
        out[surface] = groups
    return out


def _on_device(cases):
    """-> (frames: tuples of CUDA views, [(device buffer, host copy)])"""
    import torch
    frames, keep = [], []
    for lay, buf, _ in cases:
        d = torch.from_numpy(buf).cuda()
        frames.append(lay.torch_views(d))
        keep.append((d, buf))
    return frames, keep


def _unchanged(keep):
    for d, host in keep:
        assert np.array_equal(d.cpu().numpy(), host), "the call wrote into a source buffer"


# ---- every size, surface and mode: one submission of mixed sizes and layouts per matrix ----
@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("surface", ym.SURFACES)
def test_sizes_surfaces_modes(enc, expected, sweep, surface, flags):
    for k, cases in sweep[surface].items():
        frames, keep = _on_device(cases)
        pngs = enc.encode_yuv(frames, surface=surface, matrix=ym.matrix(*MATRICES[k]), flags=flags)
        assert len(pngs) == len(cases)
        for png, (lay, _, rgb) in zip(pngs, cases):
            _same(png, expected(rgb, flags), f"{surface} {lay.w} x {lay.h} pitch {lay.pitch} chroma {lay.chroma_offset} luma at {lay.luma} flags {flags}")
        _unchanged(keep)


# ---- every layout at the window and super-window edges ----
@pytest.mark.parametrize("surface", ym.SURFACES)
def test_every_layout(enc, expected, surface):
    cases = []
    for j, layout in enumerate(LAYOUTS):
        for i, (w, h) in enumerate([(65, 4), (257, 3), (520, 5)]):
            lay, buf, rgb, _ = _case(surface, w, h, layout, 3 * (7 * j + i), (i + j) % 3)  # (seed % 3 == 0: one matrix for the call)
            cases.append((lay, buf, rgb))
    frames, keep = _on_device(cases)
    for flags in (0, 1):
        pngs = enc.encode_yuv(frames, surface=surface, matrix=ym.matrix(*MATRICES[0]), flags=flags)
        for png, (lay, _, rgb) in zip(pngs, cases):
            _same(png, expected(rgb, flags), f"{surface} {lay.w} x {lay.h} pitch {lay.pitch} chroma {lay.chroma_offset} luma at {lay.luma} flags {flags}")
    _unchanged(keep)


def test_standard_and_range_arguments(enc, expected):
    """matrix=None: yuv_matrix(standard, full_range); a column swap serves NV21"""
    lay, buf, _, _ = _case("nv12", 130, 6, LAYOUTS[0], 5, 2)
    planes = lay.numpy_views(buf)
    frames, keep = _on_device([(lay, buf, None)])
    for standard, full_range in [("bt601", False), ("bt2020", True)]:
        (png,) = enc.encode_yuv(frames, surface="nv12", standard=standard, full_range=full_range)
        _same(png, expected(ym.to_rgb("nv12", planes, ym.matrix(standard, full_range)), 0), f"{standard} {full_range}")
    m = ym.matrix("bt709", False)
    (png,) = enc.encode_yuv(frames, surface="nv12", matrix=m[:, [0, 2, 1, 3]])
    swapped = (planes[0], planes[1][..., ::-1])
    _same(png, expected(ym.to_rgb("nv12", swapped, m), 0), "NV21 as a column swap")
    _unchanged(keep)


# ---- next to the other kinds on one encoder ----
def test_in_flight_next_to_a_plain_and_a_float_submission(enc, expected, sweep):
    import torch
    import fpng_amd
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (40, 333, 3), dtype=np.uint8)
    flt = rng.random((3, 37, 130), dtype=np.float32)
    cases = sweep["p016"][0]
    frames, keep = _on_device(cases)
    cap = lambda w, h: torch.empty(fpng_amd.max_encoded_size(w, h, 3) + 64, dtype=torch.uint8, device="cuda")  # noqa: E731
    o_img, o_flt, o_yuv = [cap(333, 40)], [cap(130, 37)], [cap(lay.w, lay.h) for lay, _, _ in cases]
    t_img, t_flt = torch.from_numpy(img).cuda(), torch.from_numpy(flt).cuda()
    enc.submit([t_img], o_img)
    tk_img = enc.last_ticket
    n = enc.submit_yuv(frames, outs=o_yuv, surface="p016", matrix=ym.matrix(*MATRICES[0]), flags=1)
    tk_yuv = enc.last_ticket
    enc.submit_float([t_flt], o_flt)
    tk_flt = enc.last_ticket
    assert n == len(cases) and tk_img < tk_yuv < tk_flt
    r_flt, r_yuv, r_img = enc.wait(tk_flt, 1), enc.wait(tk_yuv, n), enc.wait(tk_img, 1)
    assert enc.query(tk_yuv)
    for (size, _, status), out, (lay, _, rgb) in zip(r_yuv, o_yuv, cases):
        assert status == 0
        _same(bytes(out[:size].cpu().numpy()), expected(rgb, 1), f"p016 {lay.w} x {lay.h} between two other submissions")
    _same(bytes(o_img[0][:r_img[0][0]].cpu().numpy()), expected(img, 0), "the plain submission")
    q = np.rint(np.clip(flt.astype(np.float32) * np.float32(255.0), 0, 255)).astype(np.uint8).transpose(1, 2, 0)
    _same(bytes(o_flt[0][:r_flt[0][0]].cpu().numpy()), expected(q, 0), "the float submission")
    _unchanged(keep)


# ---- packed ----
@pytest.mark.parametrize("surface,flags,align,lead", [("nv12", 0, 16, 0), ("yuv444_16", 1, 256, 32)])
def test_packed(enc, expected, sweep, surface, flags, align, lead):
    cases = sweep[surface][0] + sweep[surface][0][:2]
    want = [expected(rgb, flags) for _, _, rgb in cases]
    sizes = [len(p) for p in want]
    cap = _need(sizes, align, lead)
    arena, pat = _arena(cap, align)
    frames, keep = _on_device(cases)
    n = enc.submit_yuv(frames, arena=arena[:cap], surface=surface, matrix=ym.matrix(*MATRICES[0]), flags=flags, align=align, lead=lead)
    recs, total = enc.wait_packed(enc.last_ticket, n)
    _check(arena, pat, recs, total, want, sizes, align, lead, cap, f"packed {surface}")
    _unchanged(keep)


# ---- renditions ----
FILTERS = ("bilinear", "bicubic", "nearest", "box", "hamming", "lanczos")


def _rendition_specs(dims):
    """per frame a thumbnail and a full-size copy; all six filters; boxes with odd origins and odd sizes"""
    specs = []
    for i, (w, h) in enumerate(dims):
        specs.append((i, (max(w // 4, 1), max(h // 4, 1)), None, FILTERS[i % 6]))
        specs.append((i, (w, h), None, "bilinear"))
    w, h = dims[0]
    for k, f in enumerate(FILTERS):
        specs.append((0, (33 + k, 17), (1 + 2 * k, 3, 97 + k, 41), f))     # odd origin
        specs.append((0, (20, 9 + k), (2 * k, 2, 61, 35 + 2 * k), f))      # even origin, odd size
    specs.append((0, (w - 1, h - 1), (1, 1, w - 1, h - 1), "bilinear"))  # a copy from an odd origin
    return specs


@pytest.mark.parametrize("surface", ["nv12", "p016", "yuv444", "yuv444_16"])
def test_renditions_are_those_of_the_converted_frame(enc, surface):
    import torch
    import fpng_amd
    dims = [(301, 77), (64, 33), (5, 3)]
    cases = [_case(surface, w, h, LAYOUTS[(i + 1) % len(LAYOUTS)], 3 * (i + 1), i % 3)[:3] for i, (w, h) in enumerate(dims)]
    frames, keep = _on_device(cases)
    rgbs = [torch.from_numpy(rgb).cuda() for _, _, rgb in cases]
    m = ym.matrix(*MATRICES[0])
    specs = _rendition_specs(dims)
    if surface in ("yuv444", "yuv444_16"):
        specs = specs[:8] + specs[-1:]
    rends = [fpng_amd.rendition(i, size, box=box, filter=f) for i, size, box, f in specs]
    for flags in (0, 1):
        want = enc.encode_renditions(rgbs, rends, kind="image", flags=flags)
        got = enc.encode_yuv(frames, renditions=rends, surface=surface, matrix=m, flags=flags)
        assert len(got) == len(want) == len(specs)
        for g, wnt, s in zip(got, want, specs):
            _same(g, wnt, f"{surface} rendition {s} flags {flags}")
    # the twin predicts the pixels: one odd-origin box against the judge's file
    lay, buf, _ = cases[0]
    px = fpng_amd.yuv_pixels([lay.numpy_views(buf)], surface=surface, matrix=m, rendition=rends[6])
    _same(got[6], _expect(np.ascontiguousarray(px), 1), f"{surface}: the twin's pixels")
    _unchanged(keep)


def test_renditions_packed(enc):
    import torch
    import fpng_amd
    dims = [(301, 77), (64, 33)]
    cases = [_case("nv12", w, h, LAYOUTS[i], 3 * i, 2)[:3] for i, (w, h) in enumerate(dims)]
    frames, keep = _on_device(cases)
    rgbs = [torch.from_numpy(rgb).cuda() for _, _, rgb in cases]
    rends = [fpng_amd.rendition(i, size, box=box, filter=f) for i, size, box, f in _rendition_specs(dims)[:8]]
    want = enc.encode_renditions(rgbs, rends, kind="image")
    sizes = [len(p) for p in want]
    cap = _need(sizes, 64, 16)
    arena, pat = _arena(cap, 64)
    n = enc.submit_yuv(frames, arena=arena[:cap], renditions=rends, surface="nv12", matrix=ym.matrix(*MATRICES[0]), align=64, lead=16)
    recs, total = enc.wait_packed(enc.last_ticket, n)
    _check(arena, pat, recs, total, want, sizes, 64, 16, cap, "packed renditions of nv12 frames")
    _unchanged(keep)
