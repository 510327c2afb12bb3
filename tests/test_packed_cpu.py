"""CPU tests of packed submissions (fpng_amd_encode_submit_packed): the placement rule fpng_amd_pack_place -- the text pack_place_kernel
compiles, csrc/pack.h -- against a sequential model written from the rule's description in include/fpng_amd.h, its properties,
fpng_amd_pack_capacity, the refusals that happen before the device is touched, and the Python helpers.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cpu_ref import ROOT

INVALID_ARG = -1
ARENA_FULL = 2
E = 0  # bytes behind png_size the chain may touch (include/fpng_amd.h, csrc/pack.h: kPackTail)
NEW_SYMBOLS = ["fpng_amd_encode_submit_packed", "fpng_amd_encode_wait_packed", "fpng_amd_pack_place", "fpng_amd_pack_capacity"]


def _up(v, a):
    return -(-v // a) * a


def model(sizes, statuses, align, lead):
    """The rule, file by file: -> (would-be offsets, extents, cursor after every file).  Whether a file fits is then
    offset + extent <= cap; a file with a status keeps offset 0 and the cursor."""
    cursor, offs, exts, cursors = 0, [], [], []
    for s, st in zip(sizes, statuses):
        off, ext = 0, _up(s + E, 16)
        if not st:
            off = _up(cursor, align) + lead
            cursor = off + ext
        offs.append(off), exts.append(ext), cursors.append(cursor)
    return np.array(offs, np.uint64), np.array(exts, np.uint64), np.array(cursors, np.uint64)


def expect(sizes, statuses, offs, exts, cap):
    """-> (offsets, statuses, total) for an arena of cap bytes"""
    sizes, statuses = np.asarray(sizes, np.uint64), np.asarray(statuses, np.uint32)
    placed = (statuses == 0) & (offs + exts <= np.uint64(cap))
    st = np.where(statuses != 0, statuses, np.where(placed, 0, ARENA_FULL)).astype(np.uint32)
    ends = np.where(placed, offs + sizes, 0)
    return np.where(placed, offs, 0).astype(np.uint64), st, int(ends[placed][-1]) if placed.any() else 0


def c_place(lib, sizes, statuses, align, lead, cap):
    n = len(sizes)
    sz = np.ascontiguousarray(sizes, np.uint64)
    st = np.ascontiguousarray(statuses if statuses is not None else [], np.uint32)
    off, st_out, total = np.zeros(n, np.uint64), np.zeros(n, np.uint32), C.c_uint64(123)
    p64, p32 = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
    rc = lib.fpng_amd_pack_place(sz.ctypes.data_as(p64), st.ctypes.data_as(p32) if statuses is not None else None, n, align, lead, cap,
                                 off.ctypes.data_as(p64), st_out.ctypes.data_as(p32), C.byref(total))
    assert rc == 0, lib.fpng_amd_last_error()
    return off, st_out, total.value


@pytest.fixture(scope="module")
def lib(built_lib):
    from fpng_amd import _lib
    return _lib.load()


def test_header_declares_and_library_exports_the_packed_calls(lib):
    from fpng_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "fpng_amd.h")).read()
    declared = set(re.findall(r"\b(fpng_amd_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW_SYMBOLS:
        assert name in declared and hasattr(lib, name) and name in _lib.SIGNATURES, name
    for macro, value in [("FPNG_AMD_DESC_IMAGE", 0), ("FPNG_AMD_DESC_EX", 1), ("FPNG_AMD_DESC_PLANAR", 2), ("FPNG_AMD_DESC_PLANAR_FLOAT", 3),
                         ("FPNG_AMD_STATUS_ARENA_FULL", 2)]:
        assert re.search(rf"#define {macro} {value}u\b", hdr), macro
    assert lib.fpng_amd_abi_version() == 5
    # the records as the header lays them out
    assert C.sizeof(_lib.Pack) == 40 and _lib.Pack.d_table.offset == 24 and _lib.Pack.lead.offset == 20
    assert C.sizeof(_lib.PackedResult) == 24 and _lib.PackedResult.status.offset == 20
    assert (_lib.DESC_IMAGE, _lib.DESC_EX, _lib.DESC_PLANAR, _lib.DESC_PLANAR_FLOAT) == (0, 1, 2, 3)


def test_pack_place_against_the_model(lib):
    """2 000 random size lists: n = 1 .. 1500, sizes 74 .. 2^33, every align and lead, incoming statuses; for each, cap = the exact
    need, one byte less, the need of the first k files, and 0.  With the properties: offsets grow, extents are disjoint and inside
    the arena, total is the last placed file's end, and behind the first refusal everything is refused."""
    rng = np.random.default_rng(20261017)
    aligns, leads = [16, 64, 512, 4096, 65536], [0, 16, 512, 65536]
    n_refused = n_with_status = 0
    for trial in range(2000):
        n = int(rng.integers(1, 1501)) if trial % 4 else int(rng.integers(1, 9))
        hi = [200, 1 << 16, 1 << 24, 1 << 33][int(rng.integers(0, 4))]
        sizes = rng.integers(74, hi + 1, n, dtype=np.uint64)
        statuses = (rng.random(n) < 0.1).astype(np.uint32) if trial % 3 == 0 else np.zeros(n, np.uint32)
        align, lead = aligns[trial % 5], leads[(trial // 5) % 4]
        offs, exts, cursors = model(sizes.tolist(), statuses.tolist(), align, lead)
        need = int(cursors[-1])
        k = int(rng.integers(0, n))
        caps = [need, max(need - 1, 0), int(cursors[k]), 0]
        n_with_status += int(statuses.any())
        for cap in caps:
            want_off, want_st, want_total = expect(sizes, statuses, offs, exts, cap)
            got_off, got_st, got_total = c_place(lib, sizes, statuses, 0 if align == 16 and trial % 2 else align, lead, cap)
            what = (trial, n, align, lead, cap)
            assert np.array_equal(got_off, want_off), what
            assert np.array_equal(got_st, want_st), what
            assert got_total == want_total, what
            # properties, on what the library answered
            placed = got_st == 0
            o, x = got_off[placed].astype(object), exts[placed].astype(object)
            assert all(o[i] + x[i] <= o[i + 1] - lead for i in range(len(o) - 1)), what  # monotonic, disjoint, the lead between them
            assert all(int(v - lead) % align == 0 for v in o), what
            assert len(o) == 0 or o[-1] + x[-1] <= cap, what
            assert got_total == (int(o[-1]) + int(sizes[placed][-1]) if len(o) else 0), what
            full = np.flatnonzero(got_st == ARENA_FULL)
            if len(full):
                n_refused += 1
                behind = got_st[full[0]:]
                assert np.all((behind == ARENA_FULL) | (statuses[full[0]:] != 0)), what
                assert not got_off[full[0]:].any(), what
            if cap == need:
                assert not len(full), what
            if cap == need - 1 and (statuses == 0).any():
                last = np.flatnonzero(statuses == 0)[-1]
                assert list(full) == [last], what  # one byte less refuses the last file, and only it
    assert n_refused > 2000 and n_with_status > 300
    # statuses = NULL means all zero
    sizes = np.array([74, 1000, 75], np.uint64)
    assert c_place(lib, sizes, None, 64, 16, 1 << 20)[0].tolist() == [16, 128 + 16, 1152 + 16]


def test_pack_capacity_is_the_rule_on_max_encoded_size(lib):
    import fpng_amd
    rng = np.random.default_rng(7)
    for trial in range(200):
        n = int(rng.integers(1, 40))
        dims = [(int(rng.integers(1, 4000)), int(rng.integers(1, 3000)), int(rng.integers(3, 5))) for _ in range(n)]
        align, lead = [16, 64, 512, 4096, 65536][trial % 5], [0, 16, 512, 65536][trial % 4]
        sizes = [fpng_amd.max_encoded_size(*d) for d in dims]
        _, _, cursors = model(sizes, [0] * n, align, lead)
        cap = fpng_amd.pack_capacity(dims, align, lead)
        assert cap == int(cursors[-1]), (dims, align, lead)
        recs, total = fpng_amd.pack_place(sizes, align, lead, cap)
        assert all(st == 0 for _, st in recs) and total == recs[-1][0] + sizes[-1]
        assert fpng_amd.pack_place(sizes, align, lead, cap - 1)[0][-1] == (0, ARENA_FULL)
    assert fpng_amd.pack_capacity([], 16, 0) == 0
    assert fpng_amd.pack_capacity([(1, 1, 3)]) == 96 and fpng_amd.pack_capacity([(1, 1, 3)], 512, 512) == 512 + 96  # (max_encoded_size = 89)


def test_refusals_before_the_device_is_touched(lib):
    """fpng_amd_encode_submit_packed checks the pack record before it looks at the encoder (no HIP call on these ways out), so the
    documented code and the reason can be seen without a GPU; the ticket stays what it was."""
    from fpng_amd import _lib
    arena = (C.c_uint8 * 4096)()
    base = _up(C.addressof(arena), 512)
    img = (_lib.Image * 1)()
    img[0].d_pixels, img[0].w, img[0].h, img[0].num_chans = base, 1, 1, 3
    pl = (_lib.ImagePlanar * 1)()
    fmt = _lib.FloatFormat()

    def submit(kind=0, images=img, fmt=None, enc=None, **kw):
        rec = dict(d_arena=base, arena_cap=1024, align=16, lead=0, d_table=None, reserved=0)
        no_pack = kw.pop("no_pack", False)
        rec.update(kw)
        pack = _lib.Pack(**rec)
        t = C.c_uint64(77)
        rc = lib.fpng_amd_encode_submit_packed(enc, kind, C.cast(images, C.c_void_p) if images is not None else None, 1, fmt, 0,
                                               None if no_pack else C.byref(pack), C.byref(t))
        assert t.value == 77
        return rc, lib.fpng_amd_last_error().decode()

    for kw, word in [(dict(kind=4), "desc_kind"), (dict(no_pack=True), "null pack"), (dict(d_arena=None), "null pack"),
                     (dict(align=24), "align"), (dict(align=8), "align"), (dict(align=131072), "align"),
                     (dict(lead=8), "lead"), (dict(lead=65536 + 16), "lead"),
                     (dict(align=512, d_arena=base + 16), "multiple of pack->align"), (dict(d_arena=base + 8), "multiple of pack->align"),
                     (dict(d_table=base + 4), "d_table"), (dict(reserved=1), "reserved"),
                     (dict(kind=0, fmt=C.byref(fmt)), "fmt"), (dict(kind=2, images=pl, fmt=C.byref(fmt)), "fmt"),
                     (dict(kind=3, images=pl), "fmt"), (dict(images=None), "null/empty")]:
        rc, why = submit(**kw)
        assert rc == INVALID_ARG and word in why, (kw, rc, why)
    # a pack record that is in order: the next thing looked at is the encoder
    for kw in [dict(), dict(align=0), dict(align=65536, d_arena=_up(base, 65536)), dict(lead=65536), dict(kind=3, images=pl, fmt=C.byref(fmt))]:
        rc, why = submit(**kw)
        assert rc == INVALID_ARG and "null encoder" in why, (kw, why)
    total = C.c_uint64(5)
    assert lib.fpng_amd_encode_wait_packed(None, 1, None, 0, C.byref(total)) == INVALID_ARG and total.value == 5
    # the host rule refuses the same align / lead values
    sz = (C.c_uint64 * 1)(100)
    for align, lead in [(24, 0), (8, 0), (131072, 0), (16, 8), (16, 65552)]:
        assert lib.fpng_amd_pack_place(sz, None, 1, align, lead, 1000, None, None, None) == INVALID_ARG
        one = (C.c_uint32 * 1)(1)
        assert lib.fpng_amd_pack_capacity(one, one, (C.c_uint32 * 1)(3), 1, align, lead) == 0
    assert lib.fpng_amd_pack_place(sz, None, 1, 16, 0, 1000, None, None, None) == 0  # (every output is optional)


def test_python_helpers_on_cpu_tensors(built_lib):
    import torch
    import fpng_amd
    from fpng_amd import Encoder
    recs, total = fpng_amd.pack_place([100, 74, 5000], 512, 512, 2048, statuses=[0, 1, 0])
    assert recs == [(512, 0), (0, 1), (0, ARENA_FULL)] and total == 612
    with pytest.raises(ValueError):
        fpng_amd.pack_capacity([(4, 4, 3)], align=48)
    with pytest.raises(fpng_amd.FpngAmdError):
        fpng_amd.pack_place([100], 16, 8, 1000)
    # descriptors without outputs, for every kind that can be laid out from a CPU tensor
    hwc = [torch.zeros(5, 7, 3, dtype=torch.uint8), torch.zeros(2, 9, 4, dtype=torch.uint8)]
    tag, kind, images, outs, arr = Encoder.make_batch_packed(hwc)
    assert (tag, kind) == ("packed", "image") and [(a.w, a.h, a.num_chans, a.d_out, a.out_cap) for a in arr] == [(7, 5, 3, None, 0), (9, 2, 4, None, 0)]
    assert arr[0].d_pixels == hwc[0].data_ptr()
    chw = torch.zeros(4, 6, 10, dtype=torch.uint8)
    _, _, _, _, arr = Encoder.make_batch_packed([chw[:3]], "planar", order="bgr")
    assert (arr[0].w, arr[0].h, arr[0].num_chans, arr[0].d_out, arr[0].out_cap) == (10, 6, 3, None, 0)
    assert arr[0].plane_pitch == -60 and arr[0].d_pixels == chw.data_ptr() + 120
    _, _, _, _, arr, fmt = Encoder.make_batch_packed([chw[:3].to(torch.float16)], "float", mean=[0.5] * 3, std=[0.25] * 3)
    assert fmt.dtype == 1 and abs(fmt.scale[0] - 63.75) < 1e-6 and arr[0].d_out is None and arr[0].row_pitch in (0, 20)
    with pytest.raises(ValueError):
        Encoder.make_batch_packed(hwc, "tar")
    with pytest.raises(ValueError):
        Encoder.make_batch_packed(hwc, "image", order="bgr")
