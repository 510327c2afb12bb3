"""The general decode tier's un-filter and pixel expansion on the CPU.  The plain model of tests/filter_writer.py is held against
Pillow on every designed file of tests/unfilter_cases.py; what those files cover is asserted from the writer's logs; the host twin
of the kernels' logic (tests/cpp/png_inflate_host.cpp, plain and with -fsanitize=address,undefined, a stand-alone program) must give
the model's pixels and the refusals' status.  The GPU tests then compare the kernels with the model alone."""
import zlib

import numpy as np
import pytest

import filter_writer as fw
import png_cases as pc
import unfilter_cases as uc
from test_png_inflate_cpu import run_twin, twins  # noqa: F401  (the fixture that builds the two twins)


@pytest.fixture(scope="module")
def reachable():
    """the Paeth classes (chosen, pa == pb, pa == pc, pb == pc) that exist: all 256^3 (a, b, c)"""
    got = fw.reachable_paeth_classes()
    assert len(got) == 10
    return got


def every_accepted():
    return uc.accepted_cases() + uc.neighbour_cases()


# ---- the model ----
def test_model_gives_pillows_pixels():
    """every accepted file loads in Pillow, and Pillow's pixels are the model's, at 3 and at 4 channels"""
    cases = every_accepted()
    assert len(cases) == 4 + 20 + 21 + 24 + 9 and len({c.name for c in cases}) == len(cases)
    for c in cases:
        for desired in (3, 4):
            exp = c.expected(desired)
            assert exp.shape == (c.h, c.w, desired), c.name
            assert np.array_equal(pc.expected(c.file, desired), exp), (c.name, desired)


def test_parity_only_files_are_exactly_the_three_pillow_refuses():
    cases = uc.parity_cases()
    assert [c.name for c in cases] == ["palette256_trns257", "grey_trns_1_byte", "rgb_trns_4_bytes"]
    for c in cases:  # (the palette file loads and fails where its tRNS is applied; the other two are refused at the chunk)
        with pytest.raises(Exception):
            pc.expected(c.file, 4)
    # what the model makes of them: 256 of the 257 bytes; no key at all
    pal, grey, rgb = cases
    assert np.array_equal(pal.expected(4)[:, :, 3], np.frombuffer(pal.trns[:256], np.uint8)[pal.recon])
    assert (grey.expected(4)[:, :, 3] == 255).all() and (rgb.expected(4)[:, :, 3] == 255).all()


def test_files_given_as_pixels_round_trip_through_the_model():
    n, cases = 0, every_accepted() + uc.parity_cases()
    for c in cases:
        assert zlib.decompress(pc.idat_stream(c.file)) == c.scan, c.name
        if c.pixels is not None:
            assert np.array_equal(c.recon, c.pixels), c.name
            n += 1
    assert n == len(cases) - 20 and all(c.pixels is None for c in uc.chain_cases())  # (the chains are given as filtered bytes)


def test_model_refuses_what_the_kernel_must_refuse():
    """each refusal differs from its accepted neighbour in one byte of the scanlines; the plain un-filter refuses the filter byte, the
    expansion the palette index, which is PLTE's entry count exactly"""
    good = {c.name: c for c in uc.neighbour_cases()}
    bad = uc.refusal_cases()
    assert len(bad) == 20 + 4 * 5 and [c.name for c in uc.neighbour_cases() if c.name.startswith("palette")][-1] == "palette256_ok"
    for c in bad:
        g = good[c.neighbour]
        assert c.status == pc.INVALID_IDAT and tuple(c) == (c.name, c.file, pc.INVALID_IDAT)
        assert zlib.decompress(pc.idat_stream(c.file)) == c.scan and len(c.scan) == len(g.scan)
        assert sum(a != b for a, b in zip(c.scan, g.scan)) == 1, c.name
        if c.name.startswith("filter_"):
            with pytest.raises(ValueError):
                fw.unfilter(c.scan, c.w, c.h, fw.BPP[c.color])
        else:
            recon = fw.unfilter(c.scan, c.w, c.h, 1)
            entries = len(c.plte) // 3
            assert (recon != g.recon).sum() == 1 and recon.max() == entries and (recon == entries).sum() == 1, c.name
            with pytest.raises(ValueError):
                fw.expand(recon, 3, c.plte, None, 4)


# ---- what the files cover, from the writer's logs ----
def test_predictor_files_meet_every_class(reachable):
    for bpp, c in zip((1, 2, 3, 4), uc.predictor_cases()):
        assert (c.w, c.h, fw.BPP[c.color]) == (70, 66, bpp) and c.log.bands == 2 and c.log.tiles == 3
        assert c.log.pred[(4, bpp)] == reachable, bpp
        assert c.log.band_top_paeth[bpp] == reachable, bpp  # (row 64: b and c come from the row the band above wrote back)
        assert c.log.pred[(3, bpp)] == fw.AVERAGE_CLASSES and len(fw.AVERAGE_CLASSES) == 8, bpp
        assert c.log.pred[(1, bpp)] == fw.WRAP_CLASSES and c.log.pred[(2, bpp)] == fw.WRAP_CLASSES, bpp
        assert uc.covers_predictors(c.log, bpp, reachable)
        assert uc.first_covering_seed(bpp, reachable) == uc.PREDICTOR_SEEDS[bpp]


def test_log_classes_follow_the_plain_predictors():
    """the log's vectorised classes against the specification's predictor on Python ints, byte by byte, on one small file"""
    c = uc.predictor_cases()[2]
    bpp, n = 3, c.w * 3
    want = {k: set() for k in (1, 2, 3, 4)}
    for y in range(c.h):
        t = c.scan[y * (n + 1)]
        for i in range(n):
            raw = c.scan[y * (n + 1) + 1 + i]
            a = int(c.recon[y, i - bpp]) if i >= bpp else 0
            b = int(c.recon[y - 1, i]) if y else 0
            cc = int(c.recon[y - 1, i - bpp]) if y and i >= bpp else 0
            if t == 1:
                want[1].add((raw + a > 255,))
            elif t == 2:
                want[2].add((raw + b > 255,))
            elif t == 3:
                want[3].add((a + b >= 256, (a + b) % 2 == 1, raw + (a + b) // 2 > 255))
            elif t == 4:
                p = a + b - cc
                pa, pb, pcc = abs(p - a), abs(p - b), abs(p - cc)
                want[4].add(("a" if pa <= pb and pa <= pcc else "b" if pb <= pcc else "c", pa == pb, pa == pcc, pb == pcc))
    assert {k: c.log.pred[(k, bpp)] for k in want} == want


def test_paeths_first_tie_decides_no_value():
    """pa == pb with a != b means a + b == 2c, so pc == 0 and c is chosen; with a == b either choice is the same byte.  `pa < pb` in
    place of `pa <= pb` is therefore the same function, and no file can tell them apart: nobody need look for one.  The second
    comparison (pb <= pc) does decide values, and class ('b', False, False, True) is where."""
    b, c = np.meshgrid(np.arange(256, dtype=np.int64), np.arange(256, dtype=np.int64), indexing="ij")
    second = 0
    for a in range(256):
        p = a + b - c
        pa, pb, pcc = abs(p - a), abs(p - b), abs(p - c)
        spec = np.where((pa <= pb) & (pa <= pcc), a, np.where(pb <= pcc, b, c))
        assert np.array_equal(spec, np.where((pa < pb) & (pa <= pcc), a, np.where(pb <= pcc, b, c)))
        second += int((spec != np.where((pa <= pb) & (pa <= pcc), a, np.where(pb < pcc, b, c))).sum())
    assert second > 0


def test_chain_files_are_constant_filtered_bytes():
    cases = uc.chain_cases()
    consts = set()
    for filt in (1, 2, 3, 4):
        for bpp in (1, 2, 3, 4):
            c, = [c for c in cases if c.name.startswith(f"chain_f{filt}_bpp{bpp}_")]
            rows = np.frombuffer(c.scan, np.uint8).reshape(c.h, -1)
            assert (c.w, c.h) == (200, 70) and (rows[:, 0] == filt).all() and len(set(rows[:, 1:].reshape(-1).tolist())) == 1
            consts.add(int(rows[0, 1]))
            assert set(c.log.pred) == {(filt, bpp)}
    assert consts == {0x01, 0x80, 0xFF}
    for bpp in (1, 2, 3, 4):
        c, = [c for c in cases if c.name == f"chain_random_bpp{bpp}"]
        assert {k for k, _ in c.log.pred} == {0, 1, 2, 3, 4}


def test_shape_files_reach_what_they_are_listed_for():
    cases = uc.shape_cases()
    assert [c.dims for c in cases] == [(w, h) for h in (64, 65) for w in (127, 128, 129, 130)] + [(70, h) for h in (127, 128, 191, 192, 193)] + [
        (4097, 3), (40000, 1), (8200, 2), (1, 4097), (2, 4097), (3, 1000), (1000, 128), (1000, 129)]
    assert [c.color for c in cases[:13]] == [0, 4, 2, 6, 3, 0, 4, 2, 6, 3, 0, 4, 2] and [c.color for c in cases[13:]] == [6, 0, 6, 0, 4, 2, 2, 2]
    for c in cases:
        r, log = c.reaches, c.log
        assert r and (log.bands, log.tiles) == (r["bands"], r["tiles"]), c.name
        assert r.get("positions", set()) <= log.positions and not r.get("not_positions", set()) & log.positions, c.name
        assert {"x=0", "y=0"} <= log.positions
        if "last_steps" in r:
            assert r["last_steps"] in log.last_steps, c.name
        if "row_bytes_above" in r:
            assert log.row_bytes > r["row_bytes_above"], c.name
        assert {k for k, _ in log.pred} >= ({0, 1, 2, 3, 4} if c.h >= 64 else set()), c.name  # (a random type per row)
    by = {c.dims: c.log for c in cases}
    # (w + 63 steps in a full band: 62, 63, 0 and 1 past a tile's edge)
    assert [by[(w, 64)].last_steps for w in (127, 128, 129, 130)] == [{61}, {62}, {63}, {0}]
    assert by[(8200, 2)].row_bytes + 1 == 32801


def test_expansion_files_hold_what_the_table_lists():
    cases = {c.name: c for c in uc.expansion_cases()}
    for key in uc.GREY_KEYS:
        c = cases[f"grey_key_{key:04x}"]
        assert set(c.recon.reshape(-1).tolist()) == set(range(256)) and c.trns == bytes([key >> 8, key & 255])
        assert ((c.expected(4)[:, :, 3] == 0) == (c.recon == (key & 255))).all() and (c.expected(4)[:, :, 3] == 0).any()
    for r, g, b, hi in uc.RGB_KEYS:
        c = cases[f"rgb_key_{r}_{g}_{b}_hi{hi:02x}"]
        px, key = c.recon.reshape(c.h, c.w, 3), np.array([r, g, b])
        assert c.trns == bytes([hi, r, hi, g, hi, b])
        same = px == key
        for rows in (slice(0, 64), slice(64, None)):
            for x in (0, c.w - 1):
                col, eq = px[rows, x], same[rows, x]
                assert eq.all(axis=1).any(), (c.name, x)
                for pair in ((0, 1), (0, 2), (1, 2)):  # equal to the key in exactly these two channels
                    other = 3 - sum(pair)
                    assert (eq[:, pair[0]] & eq[:, pair[1]] & ~eq[:, other]).any(), (c.name, x, pair)
                for perm in ((r, b, g), (g, r, b), (g, b, r), (b, r, g), (b, g, r)):
                    assert (col == np.array(perm)).all(axis=1).any(), (c.name, x, perm)
        assert ((c.expected(4)[:, :, 3] == 0) == same.all(axis=2)).all()
    ga = cases["grey_alpha_edges"].recon.reshape(70, -1, 2)
    assert {(int(g), int(a)) for g, a in ga.reshape(-1, 2)} >= {(g, a) for g in (0, 255) for a in (0, 1, 254, 255)}
    assert [len(cases[f"palette256_trns{n}"].trns) for n in (0, 1, 255, 256)] == [0, 1, 255, 256] and len(cases["palette256_trns0"].plte) == 768
    assert len(cases["palette10_trns20"].plte) == 30 and len(cases["palette10_trns20"].trns) == 20

    def chunk_types(file):
        at, out = 8, []
        while at + 12 <= len(file):
            out.append(file[at + 4:at + 8])
            at += 12 + int.from_bytes(file[at:at + 4], "big")
        return out

    assert chunk_types(cases["trns_in_front_of_plte"].file) == [b"IHDR", b"tRNS", b"PLTE", b"IDAT", b"IEND"]
    assert chunk_types(cases["two_plte_chunks"].file) == [b"IHDR", b"PLTE", b"PLTE", b"IDAT", b"IEND"]
    for name, color, kind in (("plte_in_rgb", 2, b"PLTE"), ("plte_in_rgb_not_multiple_of_3", 2, b"PLTE"), ("plte_in_rgba", 6, b"PLTE"), ("trns_in_grey_alpha", 4, b"tRNS"), ("trns_in_rgba", 6, b"tRNS")):
        assert cases[name].color == color and chunk_types(cases[name].file) == [b"IHDR", kind, b"IDAT", b"IEND"]
    at = cases["plte_in_rgb_not_multiple_of_3"].file.index(b"PLTE")
    assert int.from_bytes(cases["plte_in_rgb_not_multiple_of_3"].file[at - 4:at], "big") % 3
    assert [cases[n].channels for n in ("palette256_trns0", "palette256_trns1", "trns_in_front_of_plte", "two_plte_chunks", "trns_in_grey_alpha", "trns_in_rgba")] == [3, 4, 4, 3, 2, 4]


def test_scanlines_stay_under_a_mebibyte():
    assert max(len(c.scan) for c in every_accepted() + uc.refusal_cases() + uc.parity_cases()) <= uc.MAX_SCAN


# ---- the host twin ----
@pytest.mark.parametrize("which", ["plain", "sanitizers"])
@pytest.mark.parametrize("desired", [3, 4])
def test_host_twin_gives_the_models_pixels(twins, which, desired):
    plain, san, d = twins
    cases = every_accepted() + uc.parity_cases()
    got = run_twin(plain if which == "plain" else san, d, [c.file for c in cases], desired, f"unfilter{desired}")
    for c, (status, w, h, chans, hsh, guard) in zip(cases, got):
        assert status == 0 and (w, h) == c.dims, c.name
        assert hsh == pc.pixel_hash(c.expected(desired).tobytes()), c.name
        assert chans == c.channels and guard == 1, c.name


@pytest.mark.parametrize("which", ["plain", "sanitizers"])
def test_host_twin_refuses_by_position(twins, which):
    plain, san, d = twins
    cases = uc.refusal_cases()
    got = run_twin(plain if which == "plain" else san, d, [c.file for c in cases], 4, "unfilter_refused")
    for c, (status, _, _, _, _, guard) in zip(cases, got):
        assert status == pc.INVALID_IDAT, c.name
        assert guard == 1, c.name
