"""Streams built token by token (deflate_writer.py) for the general decode tier's inflate: the edges of its tables, of its emit step
and of its bit reader that zlib's own output never reaches, the refusals that belong to them, and a seeded random corpus
(test_png_inflate_streams_cpu.py, test_gpu_decode_png_streams.py).  Every file is grey and one row high: with filter byte 0 the
pixels are inflate's output behind its first byte, so a wrong pixel points at inflate."""
import collections
import functools
import random

import deflate_writer as dw
import png_cases as pc
from deflate_writer import dynamic, fixed, raw, stored

# name; the .png; the bytes the stream means; the writer's log; (w, h); the IDAT payloads' sizes; pixels == data[1:w + 1]
Case = collections.namedtuple("Case", "name file data log dims idat plain")

LEN_EDGES = (63, 64, 65, 127, 128, 129, 192, 193, 257, 258)
DIST_EDGES = (1, 2, 3, 63, 64, 65)
IDAT_EDGES = (8, 9, 15, 16, 17)
TOKEN_COUNTS = (0, 1, 63, 64, 65, 127, 128, 129)


def _pieces(stream, idat):
    """idat: None (one chunk), a list of sizes (repeated), or the payloads themselves"""
    if idat is None:
        return [stream]
    if idat and isinstance(idat[0], (bytes, bytearray)):
        assert b"".join(idat) == stream
        return list(idat)
    return pc.split(stream, idat)


def case(name, blocks, idat=None, width=None, **kw):
    stream, data, log = dw.write(blocks, **kw)
    pieces = _pieces(stream, idat)
    w = len(data) - 1 if width is None else width
    return Case(name, pc.png(w, 1, 0, stream, idat=pieces), data, log, (w, 1), [len(p) for p in pieces], data[0] == 0)


def _noise(rng, n, first=None):
    b = bytearray(rng.randrange(256) for _ in range(n))
    if first is not None and n:
        b[0] = first
    return bytes(b)


# ---- designed, accepted ----
def _table_cases(rng):
    out = []
    # literal/length codes of 9, 10, 11, 12 and 15 bits on symbols the tokens use: 10 bits is the fast table's last length
    lit = dw.fill_code({0: 2, 256: 3, 97: 9, 98: 10, 99: 11, 100: 12, 101: 15, 102: 15, 257: 10, 258: 11, 285: 15}, 286)
    toks = [0, 97, 98, 99, 100, 101, 102, (3, 1), (4, 2), 98, 99, (3, 2), 101, (4, 1), (258, 5), 102, 97]
    out.append(case("lit_codes_10_11_15", [dynamic(toks, lit)]))
    # distance codes of 8 .. 15 bits
    dist = dw.fill_code({0: 8, 1: 9, 2: 10, 3: 11, 4: 12, 5: 13, 6: 14, 7: 15, 8: 15}, 30)
    toks = [0] + list(_noise(rng, 20))
    for d in (1, 2, 3, 4, 5, 7, 9, 13, 17, 6, 8, 12, 16, 24):
        toks += [(3 + d % 5, d), rng.randrange(256)]
    out.append(case("dist_codes_8_to_15", [dynamic(toks, None, dist)]))
    # a code length code with 7-bit codes, all of them sent
    lit = dw.random_code(set(range(0, 286, 3)) | {256}, 15, rng, 286, deep=0.9)
    cl = set(lit) | {1}
    assert len(cl) >= 9
    clc = dw.random_code(cl, 7, rng, 19, deep=1.0)
    assert max(clc) == 7
    toks = list(range(0, 256, 3)) + [(n, 1 + n % 2) for n in (4, 7, 10, 15, 23, 35, 59, 99, 163, 258)]  # (length symbols 258, 261 .. 285)
    out.append(case("clc_7_bits", [dynamic(toks, lit, [1, 1], clc_lens=clc)]))
    # HLIT 29, HDIST 29, HCLEN 19: 286 + 30 codes, thirty distance codes, and the last code length code length (symbol 15's) sent
    lit = dw.random_code(range(286), 15, rng, 286, deep=0.9)
    dist = dw.random_code(range(30), 15, rng, 30, deep=0.6)
    assert 15 in lit
    toks = list(_noise(rng, 40)) + [(258, 24577), (258, 32768), (3, 1), 7, (200, 16385)] + [(5, dw.DIST_BASE[s]) for s in range(30)]
    out.append(case("hlit29_hdist29_hclen19", [stored(_noise(rng, 32768, 0)), dynamic(toks, lit, dist, hclen=19)]))
    assert out[-1].log["blocks"][1]["hclen"] == 19
    # a symbol 16 that begins in the literal/length lengths and ends in the distance lengths; the last repeat ends at the total
    lit = [1] + [0] * 252 + [4, 4, 3, 3, 3]
    cl = [1, (18, 138), (18, 114), 4, 4, 3, (16, 6), (16, 4)]
    toks = [0, 253, 254, 255, 0, 0, 253] + [(3, d) for d in (1, 2, 3, 4, 5, 7, 9, 13)] + [255, (3, 16)]
    out.append(case("repeat_16_crosses_tables", [dynamic(toks, lit, [3] * 8, cl_syms=cl)]))
    for sym, zeros in ((17, 3), (17, 10), (18, 11), (18, 28)):
        lit = dw.flat_code([0] + list(range(251, 258)), 258)
        cl = [3, (18, 138), (18, 112)] + [3] * 7 + [1, 1, (sym, zeros)]
        out.append(case(f"repeat_{sym}_of_{zeros}_ends_at_total", [dynamic([0, 251, 252, (3, 1), 253, (3, 2), 255], lit, [1, 1] + [0] * zeros, cl_syms=cl)]))
    # the distance code's short forms
    out.append(case("literals_hdist0_length0", [dynamic([0] + list(_noise(rng, 90)), None, [0])]))
    out.append(case("single_distance_code_symbol_0", [dynamic([0, 9, (10, 1), 8, (3, 1), (258, 1)], None, [1])]))
    out.append(case("single_distance_code_symbol_29", [stored(_noise(rng, 32768, 0)), dynamic([1, 2, (5, 24577), 3, (258, 32768), (64, 30000)], None, [0] * 29 + [1])]))
    # the end-of-block symbol alone, a single 1-bit code: in mid-stream and as the final block
    eob_only = dict(lit_lens=[0] * 256 + [1], dist_lens=[0])
    out.append(case("eob_only_in_mid_stream", [fixed([0, 1, 2, 3]), dynamic([], **eob_only), fixed([4, 5, (4, 6)])]))
    out.append(case("eob_only_final", [fixed([0, 1, 2, 3, (9, 2)]), dynamic([], **eob_only)]))
    out.append(case("eob_only_with_distance_codes", [stored(_noise(rng, 5, 0)), dynamic([], [0] * 256 + [1], [2, 2, 2, 2]), dynamic([], [0] * 256 + [1], [1]), fixed([7])]))
    return out


def _symbol_cases(rng):
    out = []
    # every length symbol at its lowest and highest extra value, in the fixed code and in a random one
    lens = sorted({v for k in range(29) for v in (dw.LENGTH_BASE[k], dw.LENGTH_BASE[k] + (1 << dw.LENGTH_EXTRA[k]) - 1)})
    toks = [0] + list(_noise(rng, 30))
    for k, n in enumerate(lens):
        toks += [(n, 1 + (k * 7) % 31), rng.randrange(256)]
    toks += [(258, 17, 284), 5, (258, 1, 284)]
    out.append(case("length_symbols_fixed", [fixed(toks)]))
    lit = dw.random_code({t for t in toks if isinstance(t, int)} | set(range(256, 286)), 15, rng, 286, deep=0.5)
    out.append(case("length_symbols_dynamic", [dynamic(toks, lit, dw.random_code(range(10), 9, rng, 10))]))
    # every distance symbol at its lowest and highest extra value, behind 32768 stored bytes
    toks = []
    for k in range(30):
        for d in (dw.DIST_BASE[k], dw.DIST_BASE[k] + (1 << dw.DIST_EXTRA[k]) - 1):
            toks += [(3 + (d % 9), d), rng.randrange(256)]
    out.append(case("distance_symbols_fixed", [stored(_noise(rng, 32768, 0)), fixed(toks)]))
    out.append(case("distance_symbols_dynamic", [stored(_noise(rng, 32768, 0)), dynamic(toks, None, dw.random_code(range(30), 15, rng, 30, deep=0.8))]))
    return out


def _emit_cases(rng):
    out = []
    # the rounds of 64 against distances that wrap several times in a round
    toks = []
    for n in LEN_EDGES:
        for d in DIST_EDGES:
            toks += [(n, d), rng.randrange(256), rng.randrange(256)]
    out.append(case("round_lengths_at_small_distances", [stored(_noise(rng, 70, 0)), fixed(toks)]))
    # batches: exactly 64 tokens; a match in slot 63; 64 matches; 65 tokens
    out.append(case("batch_of_64_literals", [fixed([0] + list(_noise(rng, 63)))]))
    out.append(case("match_in_slot_63", [fixed([0] + list(_noise(rng, 62)) + [(130, 3)])]))
    out.append(case("match_in_slot_63_then_more", [dynamic([0] + list(_noise(rng, 62)) + [(65, 63), 1, (64, 64), 2])]))
    toks = [(3 + (k * 37) % 256, 1 + (k * 5) % 9) for k in range(64)]
    out.append(case("batch_of_64_matches", [stored(_noise(rng, 10, 0)), fixed(toks)]))
    out.append(case("two_batches_of_64_matches", [stored(_noise(rng, 10, 0)), dynamic(toks + [(n, 1 + (d * 3) % 200) for n, d in toks])]))
    # sources produced earlier in the same batch: by literals, by a match, by the match in front
    out.append(case("source_in_same_batch", [fixed([0, 1, 2, 3, (6, 3), (20, 9), (258, 29), 9, (100, 258), (64, 100), (3, 3), (3, 3), (129, 6)])]))
    # distance == output so far, in the first batch, in a later one and across a block boundary
    toks, n = [0] + list(_noise(rng, 9)), 10
    for length in (5, 64, 3, 258, 129):
        toks += [(length, n), rng.randrange(256)]
        n += length + 1
    toks += list(_noise(rng, 70))
    n += 70
    toks += [(65, n), (3, n + 65)]
    out.append(case("distance_equals_output_so_far", [fixed(toks), dynamic([(258, n + 68), 4, (7, n + 68 + 259)])]))
    # sources and destinations across 32768 and 65536
    blocks = [stored(_noise(rng, 32768 - 100, 0)), fixed([(258, 50), (258, 300), 1, (258, 32768), (200, 32767)])]
    n = 32768 - 100 + 258 * 3 + 1 + 200
    blocks += [stored(_noise(rng, 65536 - 130 - n)), dynamic([(258, 32768), (193, 200), 2, (258, 32700), (129, 1)])]
    out.append(case("matches_across_32768_and_65536", blocks, idat=[4000]))
    # a match that straddles the image's last byte: output beyond the image is inflated, checked and not stored
    c = case("match_straddles_scan_bytes", [stored(_noise(rng, 300, 0)), fixed([(258, 290), 3, (100, 1)])], width=300 + 100 - 1)
    out.append(c._replace(plain=False))
    out.append(case("length_258_as_symbol_284", [stored(_noise(rng, 40, 0)), fixed([(258, 33, 284), 1, (258, 1, 284)]), dynamic([(258, 2, 284), 2, (258, 300, 284), (258, 3)])]))
    return out


def _reader_cases(rng):
    out = []
    # IDAT payloads around pngi_refill's change of path at 8 bytes left
    blocks = random_blocks(random.Random(77), 1500)
    for sizes in ([8], [9], [15], [16], [17], [17, 8, 16, 9, 15, 1, 7]):
        out.append(case("idat_payloads_of_" + "_".join(map(str, sizes)), blocks, idat=sizes))
    # a stored block over several small chunks, an empty one inside it
    blocks = [fixed([0, 1, 2]), stored(_noise(rng, 100)), fixed([3, 4, (5, 50)])]
    s, _, log = dw.write(blocks)
    a = 2 + log["blocks"][1]["end_bit"] // 8 - 100  # (the stored block's data: bytes a .. a + 100 of the stream)
    assert s[a - 4:a - 2] == b"\x64\x00"
    cuts = [0, 3, a - 2, a - 2, a + 1, a + 1, a + 6, a + 30, a + 30, a + 30, a + 79, a + 100, len(s)]  # (an empty chunk inside NLEN too)
    out.append(case("stored_over_small_chunks", blocks, idat=[s[a:b] for a, b in zip(cuts, cuts[1:])]))
    # a stored block behind a Huffman block that ends at each bit offset: the reader then holds whole bytes of the stored block, with
    # LEN 0, 1 and 2 more than the block needs.  In the fixed code a literal below 144 has 8 bits, one above 9.
    for nine in range(8):
        for length in (0, 1, 2, 9):
            eight = 2 + (3 * nine + length) % 7
            toks = [0] + [rng.randrange(144) for _ in range(eight - 1)] + [200 + k for k in range(nine)]
            blocks = [fixed(toks), stored(_noise(rng, length)), fixed([1, 2, (3, 2), 250])]
            idat = None if (nine + length) % 2 else [5]
            out.append(case(f"stored_behind_bit_{(2 + nine) % 8}_len_{length}", blocks, idat=idat))
    return out


def _filter_cases(rng):
    """the same kind of stream with filter bytes 1 - 4 (a row of one-byte pixels: Pillow's pixels are the expectation)"""
    out = []
    for f in (1, 2, 3, 4):
        c = case(f"filter_{f}", [fixed([f] + list(_noise(rng, 70)) + [(100, 7)]), stored(_noise(rng, 30)), dynamic([5, (64, 64), 6])], idat=[16])
        out.append(c._replace(plain=False))
    return out


@functools.lru_cache(None)
def accepted_cases():
    rng = random.Random(2024)
    return _table_cases(rng) + _symbol_cases(rng) + _emit_cases(rng) + _reader_cases(rng) + _filter_cases(rng)


# ---- designed, refused: (name, file, status); test_png_inflate_streams_cpu.py holds each against zlib ----
TRUNCATED = ("stored_len_past_last_idat",)  # refused because the input ends: zlib's decompressobj reports that with eof == False


@functools.lru_cache(None)
def refused_cases():
    out = []

    def refuse(name, blocks, **kw):
        kw.setdefault("pad", 8)
        kw.setdefault("adler", False)
        c = case(name, blocks, width=8, **kw)
        out.append((name, c.file, pc.INVALID_IDAT))

    lead = fixed([0, 1, 2, 3, 4, 5, 6, 7, 8])  # the image's nine bytes
    some = [0, 1, 2, 3, 4, 5, 6, 7, 8, (3, 1)]
    # HLIT / HDIST 30 and 31: streams that hold together -- as many lengths are sent as the header says, the ones past 286 / 30
    # are zeros, the codes are complete -- so that only the range check can refuse them
    well = dynamic(some + [(3, 2)])
    assert dw.kraft(well["lit_lens"]) == 32768 and well["dist_lens"] == [1, 1]
    for v in (30, 31):
        lit = well["lit_lens"] + [0] * (257 + v - len(well["lit_lens"]))
        refuse(f"hlit_{v}", [dynamic(well["tokens"], lit, [1, 1], check=False)])
        refuse(f"hdist_{v}", [dynamic(well["tokens"], well["lit_lens"], [1, 1] + [0] * (v - 1), check=False)])
    eob = [0] * 256 + [1]
    refuse("repeat_past_total", [lead, dynamic([], eob, [0], cl_syms=[(18, 138), (18, 118), 1, (17, 3)], check=False)])
    refuse("repeat_16_past_total", [lead, dynamic([], eob, [0], cl_syms=[(18, 138), (18, 118), 1, (16, 3)], check=False)])
    refuse("single_distance_code_unused_code", [dynamic(some[:9] + [(3, raw(1, 1))], None, [1])])
    refuse("distance_code_two_codes_incomplete", [lead, dynamic([1, 2], None, [2, 2])])
    refuse("distance_past_start_in_second_batch", [fixed(list(range(70)) + [(3, 71)])])
    refuse("distance_past_start_by_one_after_matches", [fixed(list(range(64)) + [(100, 64), (3, 165)])])
    refuse("single_distance_code_of_length_2", [lead, dynamic([1, 2], None, [2])])
    refuse("distance_code_oversubscribed", [lead, dynamic([1, 2], None, [1, 1, 1])])
    refuse("length_symbol_without_distance_code", [dynamic(some[:9] + [(3, raw(0, 1))], None, [0])])
    refuse("clc_one_1_bit_code", [lead, dynamic([], [8] * 257, [8], clc_lens=[0] * 8 + [1] + [0] * 10, check=False)])
    refuse("stored_len_past_last_idat", [lead, stored(bytes(10), len_field=100)], pad=0)
    refuse("eob_only_unused_code", [lead, dynamic([raw(1, 1)], eob, [0])])
    return out


# ---- one documented leniency, one case of parity only ----
@functools.lru_cache(None)
def window_cases():
    """a match at distance 700 under a header that declares a 512-byte window, and the same body under CINFO 7"""
    rng = random.Random(5)
    blocks = [stored(_noise(rng, 800, 0)), fixed([(258, 700), 1, (30, 513), (3, 512)])]
    return case("window_512_distance_700", blocks, cinfo=1), case("window_32768_distance_700", blocks, cinfo=7)


@functools.lru_cache(None)
def ends_on_last_bit_case():
    """the final end-of-block symbol's last bit is the last bit of the last IDAT byte; no Adler-32 follows"""
    c = case("ends_on_last_bit", [fixed([0, 1, 2, 3] + [200 + k for k in range(6)])], adler=False)
    assert c.log["blocks"][0]["end_bit"] % 8 == 0 and c.idat == [2 + c.log["blocks"][0]["end_bit"] // 8]
    return c


# ---- seeded random ----
def _random_dynamic(rng, toks):
    lit_used = {256} | {t for t in toks if isinstance(t, int)} | {t[2] if len(t) > 2 else dw.length_symbol(t[0]) for t in toks if isinstance(t, tuple)}
    extra = rng.choice((0, 0, 3, 40, 286))
    if extra:
        lit_used |= set(rng.sample(range(286), extra))
    lit = dw.random_code(lit_used, 15, rng, 286, deep=rng.choice((0.0, 0.3, 0.8, 0.97)))
    lit = lit[:rng.randint(max(257, max(lit_used) + 1), 286)]
    dist_used = {dw.dist_symbol(t[1]) for t in toks if isinstance(t, tuple)}
    extra = rng.choice((0, 0, 1, 5, 30))
    if extra:
        dist_used |= set(rng.sample(range(30), extra))
    if not dist_used:
        dist = [0]
    else:
        dist = dw.random_code(dist_used, 15, rng, 30, deep=rng.choice((0.0, 0.5, 0.95)))
        dist = dist[:rng.randint(max(dist_used) + 1, 30)]
    if not any(dist) and rng.random() < 0.5:
        dist = [0] * rng.randint(1, 30)
    cl = dw.random_cl(lit + dist, rng, repeats=rng.choice((0.0, 0.5, 0.9, 1.0)))
    cl_used = {t[0] if isinstance(t, tuple) else t for t in cl}
    if len(cl_used) < 2 or rng.random() < 0.3:
        cl_used |= set(rng.sample(range(19), rng.randint(1, 6)))
    clc = dw.random_code(cl_used, 7, rng, 19, deep=rng.choice((0.0, 0.5, 1.0)))
    need = max(i + 1 for i, s in enumerate(dw.CL_ORDER) if clc[s])
    return dynamic(toks, lit, dist, cl_syms=cl, clc_lens=clc, hclen=rng.randint(max(need, 4), 19))


def random_blocks(rng, target):
    """blocks of all three kinds in random order until the output has `target` bytes or a little more; the first byte is 0"""
    blocks, n = [], 0
    big = target > 20000
    while n < target:
        kind = rng.choice(("stored", "fixed", "dynamic"))
        if len(blocks) > 40:
            kind = "stored"
        if kind == "stored":
            size = rng.choice((0, 1, 2, rng.randint(3, 300), rng.randint(300, 30000 if big else 1500)))
            if len(blocks) > 40:
                size = min(target - n, 65535)
            size = min(size, target + 100 - n)
            blocks.append(stored(_noise(rng, size, 0 if n == 0 else None)))
            n += size
            continue
        count = rng.choice(TOKEN_COUNTS + (rng.randint(2, 700 if big else 300),) * 4)
        p_lit = rng.choice((0.0, 0.2, 0.6, 0.95, 1.0))
        alphabet = rng.choice((256, 256, 20, 2))
        toks = []
        for _ in range(count):
            if n == 0:
                toks.append(0)
                n = 1
            elif rng.random() < p_lit:
                toks.append(rng.randrange(alphabet) * (255 // (alphabet - 1)) if alphabet < 256 else rng.randrange(256))
                n += 1
            else:
                length = rng.choice(LEN_EDGES + (3, 4)) if rng.random() < 0.5 else rng.randint(3, 258)
                d = rng.choice(DIST_EDGES + (257, 258, 32767, 32768)) if rng.random() < 0.5 else rng.randint(1, rng.choice((10, 300, 32768)))
                d = min(d, n, 32768)  # (a distance too far becomes the farthest there is: distance == output so far)
                toks.append((length, d, 284) if length == 258 and rng.random() < 0.3 else (length, d))
                n += length
        blocks.append(fixed(toks) if kind == "fixed" else _random_dynamic(rng, toks))
    return blocks


RANDOM_STREAMS = 300
_SPLITS = (None, [1], [7], [8], [9], [15], [16], [17], "small", [4000])


@functools.lru_cache(None)
def random_cases():
    out = []
    for seed in range(RANDOM_STREAMS):
        rng = random.Random(1000 + seed)
        target = (32768 + rng.randint(1, 300) if seed % 25 == 3 else 65536 + rng.randint(1, 300) if seed % 25 == 11 else
                  rng.randint(60000, 70000) if seed % 25 == 19 else rng.randint(50, 5000))
        split = _SPLITS[seed % len(_SPLITS)]
        if split == "small":
            split = [rng.randint(1, 40) for _ in range(rng.randint(2, 9))]
        if target > 20000 and split is not None and split[0] < 8:
            split = [split[0] + 15]  # (a chunk costs 12 bytes of file: keep the big streams' files small)
        out.append(case(f"random_{seed}", random_blocks(rng, target), idat=split))
    return out
