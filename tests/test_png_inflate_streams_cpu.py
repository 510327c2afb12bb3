"""Streams written token by token (tests/deflate_writer.py, tests/inflate_cases.py) on the CPU: the writer is held against zlib and
Pillow, what the corpus reaches is asserted from the writer's own log, and the general decode tier's host twin
(tests/cpp/png_inflate_host.cpp; plain and -fsanitize=address,undefined, a stand-alone program run as a child process) must give
Pillow's pixels for the accepted streams and INVALID_IDAT for the refused ones, which zlib refuses too."""
import functools
import zlib

import pytest

import deflate_writer as dw
import inflate_cases as ic
import png_cases as pc
from test_png_inflate_cpu import run_twin, twins  # noqa: F401  (the fixture that builds the two twins)


def accepted():
    return ic.accepted_cases() + ic.random_cases()


def body(file):
    return pc.idat_stream(file)[2:]


@functools.lru_cache(None)
def pillow_hash(name, desired):
    c = {c.name: c for c in accepted() + list(ic.window_cases())}[name]
    exp = pc.expected(c.file, desired)
    assert exp.shape[:2] == (1, c.dims[0])
    return pc.pixel_hash(exp.tobytes())


# ---- the writer against the references ----
def test_writer_means_what_zlib_reads():
    """every accepted stream, none skipped or made anew: zlib inflates the body to the bytes the writer says it means"""
    cases = accepted() + list(ic.window_cases()) + [ic.ends_on_last_bit_case()]
    assert len(ic.random_cases()) >= 300 and len(cases) >= 370
    for c in cases:
        d = zlib.decompressobj(-15)
        assert d.decompress(body(c.file)) == c.data, c.name
        assert d.eof, c.name


def test_writer_means_what_pillow_shows():
    """filter byte 0, one row of grey: the pixels are the stream's bytes behind the first"""
    plain = [c for c in accepted() if c.plain]
    assert len(plain) >= len(accepted()) - 5
    for c in plain:
        assert c.data[0] == 0 and c.dims == (len(c.data) - 1, 1)
        assert pc.expected(c.file, 3)[0, :, 0].tobytes() == c.data[1:], c.name
    for c in accepted():
        if not c.plain:
            assert pc.pillow_loads(c.file), c.name


def test_refused_streams_are_refused_by_zlib():
    """the table of refusals rests on the reference: zlib raises on each body (where the input merely ends, its streaming form
    reports that by never reaching the end of the stream, and the one-shot form raises)"""
    for name, f, status in ic.refused_cases():
        assert status == pc.INVALID_IDAT
        with pytest.raises(zlib.error):
            zlib.decompress(body(f), -15)
        d = zlib.decompressobj(-15)
        if name in ic.TRUNCATED:
            d.decompress(body(f))
            assert not d.eof, name
        else:
            with pytest.raises(zlib.error):
                d.decompress(body(f))


def test_window_case_is_refused_by_zlib_only_for_its_header():
    small, full = ic.window_cases()
    assert pc.idat_stream(small.file)[0] == 0x18 and pc.idat_stream(full.file)[0] == 0x78
    assert body(small.file) == body(full.file) and any(d == 700 for _, d, _, _, _ in small.log["matches"])
    # wbits 0: zlib keeps the window the header declares, 512 bytes.  Read in two calls (a match inside one call's output never
    # goes to the window), the distance of 700 lies outside it
    stream = pc.idat_stream(small.file)
    d = zlib.decompressobj(0)
    assert d.decompress(stream[:2 + 5 + 800]) == small.data[:800]
    with pytest.raises(zlib.error):
        d.decompress(stream[2 + 5 + 800:])
    assert zlib.decompress(pc.idat_stream(full.file)) == full.data


# ---- what the corpus reaches, from the writer's log alone ----
def _empty_chunk_inside_stored_data(c):
    """an empty IDAT, and the ends of non-empty ones on both sides of it, strictly inside one stored block's data (a stored block
    ends on a byte, its data are the bytes in front of that; the stream has two header bytes in front of the deflate data)"""
    cuts, at = [], 0
    for n in c.idat:
        cuts.append((at, n))
        at += n
    for b in c.log["blocks"]:
        if b["kind"] != "stored":
            continue
        end = 2 + b["end_bit"] // 8
        start = end - (b["out_end"] - b["out_start"])
        inside = [(p, n) for p, n in cuts if start < p < end]
        if any(n == 0 for _, n in inside) and len({p for p, _ in inside}) >= 3:
            return True
    return False


def test_coverage_of_the_corpus():
    cases = accepted()
    blocks = [(c, i, b) for c in cases for i, b in enumerate(c.log["blocks"])]
    huff = [b for _, _, b in blocks if b["kind"] != "stored"]
    dyn = [b for b in huff if b["kind"] == "dynamic"]
    matches = [(c, m) for c in cases for m in c.log["matches"]]
    # every length symbol and every distance symbol, each at its lowest and highest extra value
    lsyms = set().union(*(c.log["length_symbols"] for c in cases))
    dsyms = set().union(*(c.log["dist_symbols"] for c in cases))
    for k in range(29):
        assert {(257 + k, 0), (257 + k, (1 << dw.LENGTH_EXTRA[k]) - 1)} <= lsyms, k
    assert (284, 31) in lsyms  # length 258 the long way
    for k in range(30):
        assert {(k, 0), (k, (1 << dw.DIST_EXTRA[k]) - 1)} <= dsyms, k
    # code lengths that were used, not merely declared
    lit_used = set().union(*(b["lit_used"] for b in dyn))
    dist_used = set().union(*(b["dist_used"] for b in dyn))
    cl_used = set().union(*(b["cl_used"] for b in dyn))
    assert {1, 9, 10, 11, 12, 15} <= lit_used
    assert set(range(1, 16)) <= dist_used
    assert set(range(1, 8)) <= cl_used
    # the header's ends, repeats, the distance code's forms
    assert {0, 29} <= {b["hlit"] for b in dyn} and {0, 29} <= {b["hdist"] for b in dyn} and 19 in {b["hclen"] for b in dyn}
    assert any(b["hclen"] == 19 and 15 in b["lit_lens"] + b["dist_lens"] for b in dyn)
    assert any(b["rep16_crosses"] for b in dyn)
    assert {16, 17, 18} <= {b["ends_with_repeat"] for b in dyn}
    assert {0, 1, 30} <= {b["dist_codes"] for b in dyn}
    assert any(b["dist_codes"] == 1 and b["dist_lens"][0] == 1 and b["dist_used"] for b in dyn)
    assert any(b["dist_codes"] == 1 and len(b["dist_lens"]) == 30 and b["dist_lens"][29] == 1 and b["dist_used"] for b in dyn)
    assert any(b["dist_lens"] == [0] and b["tokens"] > 0 for b in dyn)
    # the end-of-block symbol alone: as the final block and in front of others
    eob_only = [(c, i) for c, i, b in blocks if b["kind"] == "dynamic" and b["lit_codes"] == 1 and b["lit_lens"][256] == 1]
    assert any(i == len(c.log["blocks"]) - 1 for c, i in eob_only) and any(i < len(c.log["blocks"]) - 1 for c, i in eob_only)
    # batches: a block's tokens go 64 at a time
    assert any(b["tokens"] == 64 for b in huff) and {0, 1, 63, 65, 127, 128, 129} <= {b["tokens"] for b in huff}
    assert any(ti % 64 == 63 for _, (_, _, _, _, ti) in matches)
    per_batch = {}
    for c, (_, _, _, bi, ti) in matches:
        per_batch[(c.name, bi, ti // 64)] = per_batch.get((c.name, bi, ti // 64), 0) + 1
    assert 64 in per_batch.values()
    # emit: the rounds' lengths at the small distances; distance == output so far; sources and destinations across 32768 and 65536
    pairs = {(n, d) for _, (n, d, _, _, _) in matches}
    assert {(n, d) for n in ic.LEN_EDGES for d in ic.DIST_EDGES} <= pairs
    assert any(d == pos and ti >= 64 for _, (_, d, pos, _, ti) in matches) and any(d == pos and ti < 64 for _, (_, d, pos, _, ti) in matches)
    assert {32767, 32768} <= {d for _, d in pairs}
    for edge in (32768, 65536):
        assert any(pos < edge < pos + n for _, (n, _, pos, _, _) in matches), edge             # the destination
        assert any(pos - d < edge < pos - d + min(n, d) for _, (n, d, pos, _, _) in matches), edge  # the source
    assert any(pos < c.dims[0] + 1 < pos + n for c, (n, _, pos, _, _) in matches)  # across the image's last byte
    # the reader: block ends at every bit offset in front of a stored block of 0, 1, 2 and more bytes; the IDAT payload sizes
    ends = {(a["end_bit"] % 8, b["out_end"] - b["out_start"]) for c in cases for a, b in zip(c.log["blocks"], c.log["blocks"][1:]) if a["kind"] != "stored" and b["kind"] == "stored"}
    assert {(k, n) for k in range(8) for n in (0, 1, 2)} <= ends and all(any(k == e and n > 2 for e, n in ends) for k in range(8))
    sizes = set().union(*(set(c.idat[:-1]) for c in cases))
    assert {1, 7, 4000} | set(ic.IDAT_EDGES) <= sizes and any(len(c.idat) == 1 for c in cases)
    assert any(_empty_chunk_inside_stored_data(c) for c in cases)
    # outputs from 50 bytes to 70 000, some just past 32768 and 65536
    n_out = [len(c.data) for c in ic.random_cases()]
    assert min(n_out) < 200 and max(n_out) > 60000 and any(32768 < n <= 32768 + 700 for n in n_out) and any(65536 < n <= 65536 + 700 for n in n_out)
    assert {"stored", "fixed", "dynamic"} == {b["kind"] for _, _, b in blocks}


# ---- the host twin ----
@pytest.mark.parametrize("which", ["plain", "sanitizers"])
@pytest.mark.parametrize("desired", [3, 4])
def test_accepted_streams_give_pillows_pixels(twins, which, desired):
    plain, san, d = twins
    cases = accepted()
    got = run_twin(plain if which == "plain" else san, d, [c.file for c in cases], desired, f"streams{desired}")
    for c, (status, w, h, chans, hsh, guard) in zip(cases, got):
        assert status == 0, c.name
        assert (w, h) == c.dims and chans == 1, c.name
        assert hsh == pillow_hash(c.name, desired), c.name
        assert guard == 1, c.name


@pytest.mark.parametrize("which", ["plain", "sanitizers"])
def test_refused_streams_give_their_status(twins, which):
    plain, san, d = twins
    cases = ic.refused_cases()
    got = run_twin(plain if which == "plain" else san, d, [f for _, f, _ in cases], 4, "refused")
    for (name, _, want), (status, _, _, _, _, guard) in zip(cases, got):
        assert status == want, name
        assert guard == 1, name


@pytest.mark.parametrize("which", ["plain", "sanitizers"])
def test_end_of_block_alone_is_a_code_and_its_unused_code_is_none(twins, which):
    """a literal/length code of one 1-bit code, the end-of-block symbol's, is accepted as zlib and Pillow accept it; the other
    value of that bit is no code"""
    plain, san, d = twins
    good = [c for c in ic.accepted_cases() if c.name.startswith("eob_only")]
    bad = [f for n, f, _ in ic.refused_cases() if n == "eob_only_unused_code"]
    assert len(good) == 3 and len(bad) == 1
    got = run_twin(plain if which == "plain" else san, d, [c.file for c in good] + bad, 4, "eob")
    for c, g in zip(good, got):
        assert g[0] == 0 and g[4] == pillow_hash(c.name, 4) and g[5] == 1, c.name
    assert got[-1][0] == pc.INVALID_IDAT and got[-1][5] == 1


@pytest.mark.parametrize("which", ["plain", "sanitizers"])
def test_declared_window_is_not_held_against_distances(twins, which):
    """documented leniency: the zlib header's window size is checked for its range only; a distance beyond the declared window
    but inside the output so far is taken, and gives the pixels of the same body under a 32 KiB header"""
    plain, san, d = twins
    small, full = ic.window_cases()
    got = run_twin(plain if which == "plain" else san, d, [small.file, full.file], 4, "window")
    for g in got:
        assert g[0] == 0 and g[4] == pillow_hash(full.name, 4) and g[5] == 1
    assert pc.expected(full.file, 3)[0, :, 0].tobytes() == full.data[1:]


def test_stream_that_ends_on_the_files_last_bit(twins):
    """parity only (the GPU test holds the kernels against this): both builds of the twin agree, nothing outside is touched"""
    plain, san, d = twins
    c = ic.ends_on_last_bit_case()
    a, b = run_twin(plain, d, [c.file], 4, "lastbit"), run_twin(san, d, [c.file], 4, "lastbit")
    assert a == b and a[0][5] == 1
