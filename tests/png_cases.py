"""Ordinary PNG files for the general decode tier's tests (test_png_inflate_cpu.py, test_gpu_decode_png.py): a writer of its own
(numpy filters, zlib streams with chosen parameters and flush points, IDAT chunks of chosen sizes, PLTE / tRNS / ancillary chunks),
the designed cases, the damaged ones with the status each must give, and Pillow's pixels as the expectation."""
import functools
import io
import struct
import zlib

import numpy as np

from deflate_writer import DIST_BASE, DIST_EXTRA, LENGTH_BASE, LENGTH_EXTRA, _bits, _msb

OK, NOT_FPNG, NOT_PNG, HEADER_CRC32, BAD_DIMS, CHUNK_PARSING, INVALID_IDAT, UNDECIDED, UNSUPPORTED = 0, 1, 3, 4, 5, 7, 8, 64, 67
BPP = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
SIG = b"\x89PNG\r\n\x1a\n"


def pixel_hash(data):
    """the hash tests/cpp/png_inflate_host.cpp prints: sum of (byte + 1) * ((index + 1) * 0x9E3779B97F4A7C15) mod 2^64"""
    b = np.frombuffer(bytes(data), np.uint8).astype(np.uint64)
    with np.errstate(over="ignore"):
        return int(((b + np.uint64(1)) * (np.arange(1, len(b) + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15))).sum(dtype=np.uint64))


def chunk(ctype, data=b""):
    return struct.pack(">I", len(data)) + ctype + data + struct.pack(">I", zlib.crc32(ctype + data))


def _paeth(a, b, c):
    p = a.astype(np.int32) + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filter_rows(raw, bpp, filters):
    """raw: (h, w * bpp) uint8; filters: a type 0-4 per row -> the filtered scanlines (a filter byte in front of each row)"""
    h, n = raw.shape
    out = bytearray()
    prev = np.zeros(n, np.int32)
    for y in range(h):
        cur = raw[y].astype(np.int32)
        left = np.concatenate([np.zeros(bpp, np.int32), cur[:-bpp]]) if n > bpp else np.zeros(n, np.int32)
        ul = np.concatenate([np.zeros(bpp, np.int32), prev[:-bpp]]) if n > bpp else np.zeros(n, np.int32)
        t = filters[y]
        pred = [0, left, prev, (left + prev) // 2, _paeth(left, prev, ul)][t]
        out.append(t)
        out += ((cur - pred) & 255).astype(np.uint8).tobytes()
        prev = cur
    return bytes(out)


def deflate(data, level=6, wbits=15, mem_level=8, strategy=zlib.Z_DEFAULT_STRATEGY, flushes=()):
    """flushes: (byte position of `data`, zlib.Z_FULL_FLUSH or Z_SYNC_FLUSH), ascending"""
    co = zlib.compressobj(level, zlib.DEFLATED, wbits, mem_level, strategy)
    out, at = b"", 0
    for pos, mode in flushes:
        out += co.compress(data[at:pos]) + co.flush(mode)
        at = pos
    return out + co.compress(data[at:]) + co.flush()


def split(stream, sizes):
    """the stream cut into pieces of the given sizes (the list is repeated; the rest goes into a last piece of its own)"""
    pieces, at, k = [], 0, 0
    while at < len(stream):
        n = sizes[k % len(sizes)]
        pieces.append(stream[at:at + n])
        at += n
        k += 1
    return pieces


def png(w, h, color, stream, idat=None, plte=None, trns=None, before_plte=(), after_idat=(), depth=8, interlace=0, iend=True):
    """idat: None (one chunk), a list of sizes for split(), or the list of the chunks' payloads themselves (bytes objects)"""
    f = SIG + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, color, 0, 0, interlace))
    for c in before_plte:
        f += c
    if plte is not None:
        f += chunk(b"PLTE", bytes(plte))
    if trns is not None:
        f += chunk(b"tRNS", bytes(trns))
    pieces = [stream] if idat is None else (list(idat) if idat and isinstance(idat[0], (bytes, bytearray)) else split(stream, idat))
    for p in pieces:
        f += chunk(b"IDAT", p)
    for c in after_idat:
        f += c
    return f + (chunk(b"IEND") if iend else b"")


def image(w, h, color, seed=0, kind="mix"):
    """(h, w * bpp) uint8 of some structure: smooth parts, noise and repeats, so that filters and matches all have work"""
    rng = np.random.default_rng(seed * 7919 + w * 31 + h)
    bpp = BPP[color]
    n = w * bpp
    if kind == "noise":
        return rng.integers(0, 256, (h, n), dtype=np.uint8)
    y, x = np.mgrid[0:h, 0:n]
    a = ((x * 3 + y * 5) & 255).astype(np.uint8)
    noise = rng.integers(0, 256, (h, n), dtype=np.uint8)
    pick = rng.integers(0, 4, (h, n))
    return np.where(pick == 0, noise, a).astype(np.uint8)


def make(w, h, color, filters=None, seed=0, raw=None, plte=None, trns=None, idat=None, **z):
    """a file from an image: filters = one type, a list per row, or None (a seeded random type per row)"""
    bpp = BPP[color]
    raw = image(w, h, color, seed) if raw is None else raw
    if color == 3:
        if plte is None:
            plte = np.random.default_rng(seed + 1).integers(0, 256, 768, dtype=np.uint8).tobytes()
        raw = (raw.astype(np.int32) % (len(plte) // 3)).astype(np.uint8) if len(plte) >= 3 else raw
    if filters is None:
        filters = np.random.default_rng(seed + 2).integers(0, 5, h).tolist()
    elif isinstance(filters, int):
        filters = [filters] * h
    return png(w, h, color, deflate(filter_rows(raw, bpp, filters), **z), idat=idat, plte=plte, trns=trns)


def expected(file, desired):
    """Pillow's pixels: (h, w, desired) uint8"""
    from PIL import Image
    with Image.open(io.BytesIO(file)) as im:
        return np.asarray(im.convert("RGB" if desired == 3 else "RGBA"))


def pillow_loads(file):
    from PIL import Image
    try:
        with Image.open(io.BytesIO(file)) as im:
            im.load()
        return True
    except Exception:
        return False


def idat_stream(file):
    """the concatenated IDAT payloads of a file"""
    at, out = 8, b""
    while at + 12 <= len(file):
        n, t = struct.unpack(">I4s", file[at:at + 8])
        if t == b"IDAT":
            out += file[at + 8:at + 8 + n]
        at += 12 + n
    return out


def repair_checksums(file):
    """the file with its stream's Adler-32 and every chunk's CRC recomputed, the stream in one IDAT (Pillow refuses a file over
    either checksum; the general tier reads neither)"""
    stream = idat_stream(file)
    stream = stream[:-4] + struct.pack(">I", zlib.adler32(zlib.decompressobj(-15).decompress(stream[2:])))
    at, out, placed = 8, file[:8], False
    while at + 12 <= len(file):
        n, t = struct.unpack(">I4s", file[at:at + 8])
        if t != b"IDAT":
            out += chunk(t, file[at + 8:at + 8 + n])
        elif not placed:
            out += chunk(t, stream)
            placed = True
        at += 12 + n
    return out


def max_code_length(stream):
    """the longest literal/length or distance code of the stream's FIRST block, which must be a dynamic one (RFC 1951, 3.2.7)"""
    bits = int.from_bytes(stream[2:2 + 4096], "little")
    at = 0

    def get(n):
        nonlocal at
        v = (bits >> at) & ((1 << n) - 1)
        at += n
        return v

    get(1)
    assert get(2) == 2, "not a dynamic block"
    nlit, ndist, nclc = get(5) + 257, get(5) + 1, get(4) + 4
    clc = [0] * 19
    for i in range(nclc):
        clc[(16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)[i]] = get(3)
    codes, code = {}, 0
    for ln in range(1, 8):
        for s in range(19):
            if clc[s] == ln:
                codes[(ln, code)] = s
                code += 1
        code <<= 1
    lens = []
    while len(lens) < nlit + ndist:
        code = 0
        for ln in range(1, 8):
            code = (code << 1) | get(1)
            if (ln, code) in codes:
                break
        s = codes[(ln, code)]
        if s < 16:
            lens.append(s)
        elif s == 16:
            lens += [lens[-1]] * (get(2) + 3)
        elif s == 17:
            lens += [0] * (get(3) + 3)
        else:
            lens += [0] * (get(7) + 11)
    return max(lens)


# ---- the designed cases: (name, file) lists, made once ----
def _key_image(w, h, color, key, seed):
    raw = image(w, h, color, seed)
    px = raw.reshape(h, w, BPP[color])
    px[::3, ::2] = key  # (pixels that equal the colour key, and others that share some of its bytes)
    return px.reshape(h, -1)


@functools.lru_cache(None)
def format_cases():
    out = []
    for color in (0, 2, 3, 4, 6):
        out.append((f"color{color}", make(37, 21, color, seed=color)))
    plte = np.random.default_rng(5).integers(0, 256, 3 * 200, dtype=np.uint8).tobytes()
    out.append(("palette_trns_short", make(40, 33, 3, seed=11, plte=plte, trns=bytes(range(10, 130)))))
    out.append(("palette_trns_full", make(40, 33, 3, seed=12, plte=plte, trns=bytes((i * 7) & 255 for i in range(200)))))
    out.append(("palette_small", make(19, 5, 3, seed=13, plte=plte[:9])))
    out.append(("grey_key", make(31, 17, 0, seed=14, raw=_key_image(31, 17, 0, 77, 14), trns=struct.pack(">H", 77))))
    out.append(("grey_key_16bit", make(31, 17, 0, seed=15, trns=struct.pack(">H", 0x4D4D))))
    out.append(("rgb_key", make(31, 17, 2, seed=16, raw=_key_image(31, 17, 2, (10, 200, 30), 16), trns=struct.pack(">HHH", 10, 200, 30))))
    return out


SHAPE_HEIGHTS, SHAPE_WIDTHS = (1, 2, 63, 64, 65, 129), (1, 2, 63, 64, 65, 300)


@functools.lru_cache(None)
def shape_cases():
    """heights x widths of the skewed band, EVERY shape with each filter 0-4 on every row and with a random filter per row; the
    pixel size (1, 2, 3, 4 bytes) goes round with shape and filter, so that each shape meets all four and each (filter, pixel
    size) pair nine shapes.  Then every filter with every colour type on a shape of two bands and two tiles."""
    out = []
    colors = (0, 4, 2, 6)
    for i, (h, w) in enumerate((h, w) for h in SHAPE_HEIGHTS for w in SHAPE_WIDTHS):
        for j, filt in enumerate((0, 1, 2, 3, 4, None)):
            color = colors[(i + j) % 4]
            out.append((f"shape_{w}x{h}_c{color}_f{'r' if filt is None else filt}", make(w, h, color, filters=filt, seed=6 * i + j, level=1)))
    for color in (0, 4, 2, 6, 3):
        for filt in (0, 1, 2, 3, 4, None):
            out.append((f"filter_c{color}_f{'r' if filt is None else filt}", make(70, 66, color, filters=filt, seed=300 + len(out), level=1)))
    return out


def _far_repeat_image():
    """300 x 300 RGB: noise in the first 36 rows, then copies of rows 36 rows up (32436 bytes back) with a few changed bytes:
    matches at distances near 32768 that cross rows"""
    rng = np.random.default_rng(42)
    raw = np.zeros((300, 900), np.uint8)
    raw[:36] = rng.integers(0, 256, (36, 900), dtype=np.uint8)
    for y in range(36, 300):
        raw[y] = raw[y - 36]
        raw[y, rng.integers(0, 900, 3)] ^= 0x55
    return raw


def _geometric_image(top=14, h=128):
    """byte value k 2^(top - k) times, three values once, zeros for the other half: zlib's tree reaches 15-bit codes"""
    rng = np.random.default_rng(7)
    vals = np.concatenate([np.full(2 ** (top - k), k, np.uint8) for k in range(1, top + 1)] + [np.array([top + 1, top + 2, top + 3], np.uint8)])
    w = len(vals) * 2 // h + 1
    arr = np.concatenate([vals, np.zeros(w * h - len(vals), np.uint8)])
    rng.shuffle(arr)
    return arr.reshape(h, w)


@functools.lru_cache(None)
def stream_cases():
    out = []
    raw = image(61, 40, 2, seed=3)
    scan = filter_rows(raw, 3, [y % 5 for y in range(40)])
    # stored blocks, an empty one in between (a sync flush of nothing new)
    co = zlib.compressobj(0)
    s = co.compress(scan[:3000]) + co.flush(zlib.Z_SYNC_FLUSH) + co.flush(zlib.Z_SYNC_FLUSH) + co.compress(scan[3000:]) + co.flush()
    out.append(("stored", png(61, 40, 2, s)))
    big = image(200, 150, 6, seed=4)  # 120 150 bytes: more than one 65535-byte stored block
    out.append(("stored_big", png(200, 150, 6, deflate(filter_rows(big, 4, [0] * 150), level=0))))
    for name, strat in (("fixed", zlib.Z_FIXED), ("huffman_only", zlib.Z_HUFFMAN_ONLY), ("rle", zlib.Z_RLE)):
        out.append((name, png(61, 40, 2, deflate(scan, 6, strategy=strat))))
    flat = np.zeros((50, 400), np.uint8)
    flat[:, ::97] = 9
    out.append(("rle_long_runs", png(400, 50, 0, deflate(filter_rows(flat, 1, [0] * 50), 6, strategy=zlib.Z_RLE))))
    for level in (1, 6, 9):
        out.append((f"level{level}", png(61, 40, 2, deflate(scan, level))))
    for wbits in (9, 15):
        out.append((f"wbits{wbits}", make(120, 90, 2, seed=5, level=6, wbits=wbits)))
    far = _far_repeat_image()
    out.append(("far_matches", png(300, 300, 2, deflate(filter_rows(far, 3, [0] * 300), 9))))
    geo = _geometric_image()
    out.append(("long_codes", png(geo.shape[1], geo.shape[0], 0, deflate(filter_rows(geo, 1, [0] * geo.shape[0]), 9, mem_level=9, strategy=zlib.Z_HUFFMAN_ONLY))))
    out.append(("many_blocks", png(61, 40, 2, deflate(scan, 6, flushes=[(p, zlib.Z_FULL_FLUSH if i % 2 else zlib.Z_SYNC_FLUSH) for i, p in enumerate(range(97, len(scan), 211))]))))
    return out


@functools.lru_cache(None)
def idat_cases():
    out = []
    raw = image(45, 30, 6, seed=6)
    scan = filter_rows(raw, 4, [(y * 3) % 5 for y in range(30)])
    z6 = deflate(scan, 6)
    out.append(("one_chunk", png(45, 30, 6, z6)))
    from PIL import Image
    buf = io.BytesIO()
    rng = np.random.default_rng(8)
    pic = (np.add.outer(np.arange(512), np.arange(512))[:, :, None] // np.array([2, 3, 5]) + rng.integers(0, 24, (512, 512, 3))).astype(np.uint8)
    Image.fromarray(pic, "RGB").save(buf, "PNG", compress_level=1)
    out.append(("pillow_512", buf.getvalue()))
    for n in (1, 2, 3, 7):
        out.append((f"chunks_of_{n}", png(45, 30, 6, z6, idat=[n])))
    z0 = deflate(scan, 0)
    out.append(("cut_in_zlib_header", png(45, 30, 6, z6, idat=[z6[:1], z6[1:]])))
    out.append(("cut_in_stored_len", png(45, 30, 6, z0, idat=[z0[:4], z0[4:6], z0[6:]])))
    out.append(("cut_in_adler", png(45, 30, 6, z6, idat=[z6[:-2], z6[-2:]])))
    out.append(("empty_idats", png(45, 30, 6, z6, idat=[b"", b"", z6[:100], b"", z6[100:], b"", b""])))
    text = [chunk(b"tEXt", b"Comment\0" + b"x" * 3000), chunk(b"prVt", bytes(range(256)) * 8)]
    plte = np.random.default_rng(9).integers(0, 256, 768, dtype=np.uint8).tobytes()
    idx = image(50, 40, 3, seed=10)
    out.append(("plte_behind_head", png(50, 40, 3, deflate(filter_rows(idx, 1, [4] * 40)), plte=plte, trns=bytes(range(256)), before_plte=text)))
    # output beyond the image: accepted (as Pillow accepts it), never stored
    out.append(("extra_output", png(45, 30, 6, deflate(scan + bytes(1000), 6))))
    return out


def designed_cases():
    return format_cases() + shape_cases() + stream_cases() + idat_cases() + hand_cases()


def fixed_symbol(s):
    """literal/length symbol s in the fixed code (RFC 1951, 3.2.6)"""
    return _msb(0x30 + s, 8) if s < 144 else _msb(0x190 + s - 144, 9) if s < 256 else _msb(s - 256, 7) if s < 280 else _msb(0xC0 + s - 280, 8)


def fixed_match(length, dist):
    """the fields of a match in a fixed block"""
    ls = max(k for k in range(29) if LENGTH_BASE[k] <= length and (k == 28 or length < 258))
    ds = max(k for k in range(30) if DIST_BASE[k] <= dist)
    assert 0 <= length - LENGTH_BASE[ls] < (1 << LENGTH_EXTRA[ls]) and 0 <= dist - DIST_BASE[ds] < (1 << DIST_EXTRA[ds])
    return [fixed_symbol(257 + ls), (length - LENGTH_BASE[ls], LENGTH_EXTRA[ls]), _msb(ds, 5), (dist - DIST_BASE[ds], DIST_EXTRA[ds])]


def hand_stream(matches, seed):
    """(w, h, zlib stream) of a 336 x 98 grey image built without zlib: one stored block of 32768 bytes, then a final fixed block
    of the given (length, distance) matches, 258 bytes together, which lie inside the last row.  Encoders other than zlib (which
    stops at 32506) use distances up to 32768; a match's stores then land in the window slots its own later bytes come from."""
    w, h = 336, 98
    assert sum(n for n, _ in matches) == 258 and h * (w + 1) == 32768 + 258
    rng = np.random.default_rng(seed)
    head = bytearray(rng.integers(0, 256, 32768, dtype=np.uint8).tobytes())
    for y in range(h):
        head[y * (w + 1)] = y % 5  # (the filter bytes: every type)
    fields = [(1, 1), (1, 2)]
    for n, d in matches:
        fields += fixed_match(n, d)
    body = b"\x00" + struct.pack("<HH", 32768 & 0xFFFF, ~32768 & 0xFFFF) + bytes(head) + _bits(*fields, fixed_symbol(256))
    raw = zlib.decompressobj(-15).decompress(body)
    assert len(raw) == 32768 + 258
    return w, h, b"\x78\x01" + body + struct.pack(">I", zlib.adler32(raw))


HAND_DISTANCES = (32507, 32511, 32512, 32600, 32705, 32766, 32767, 32768)


@functools.lru_cache(None)
def hand_cases():
    """hand-built streams with distances 32507 .. 32768 and lengths above 64 (one match of 258; 65 + 193; 130 + 128)"""
    out = []
    for k, d in enumerate(HAND_DISTANCES):
        w, h, z = hand_stream([(258, d)], k)
        out.append((f"hand_258_at_{d}", png(w, h, 0, z)))
    for k, d in enumerate((32767, 32705)):
        w, h, z = hand_stream([(65, d), (193, d)], 10 + k)
        out.append((f"hand_65_193_at_{d}", png(w, h, 0, z)))
        w, h, z = hand_stream([(130, d), (128, 32768)], 20 + k)
        out.append((f"hand_130_128_at_{d}", png(w, h, 0, z, idat=[4000])))
    return out


def token_stats(stream):
    """a plain inflate of a zlib stream's tokens (RFC 1951) -> (output bytes, longest distance, longest match length)"""
    data, pos = stream[2:] + bytes(8), 0

    def get(n):
        nonlocal pos
        v = (int.from_bytes(data[pos >> 3:(pos >> 3) + 4], "little") >> (pos & 7)) & ((1 << n) - 1)
        pos += n
        return v

    def table(lens):
        codes, code = {}, 0
        for ln in range(1, 16):
            for s, v in enumerate(lens):
                if v == ln:
                    codes[(ln, code)] = s
                    code += 1
            code <<= 1
        return codes

    def symbol(codes):
        code = 0
        for ln in range(1, 16):
            code = (code << 1) | get(1)
            if (ln, code) in codes:
                return codes[(ln, code)]
        raise ValueError("no code")

    out = far = longest = 0
    final = 0
    while not final:
        final, kind = get(1), get(2)
        if kind == 0:
            pos = (pos + 7) & ~7
            n = get(16)
            get(16)
            pos += 8 * n
            out += n
            continue
        if kind == 1:
            lit, dst = table([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8), table([5] * 32)
        else:
            nlit, ndist, nclc = get(5) + 257, get(5) + 1, get(4) + 4
            clc = [0] * 19
            for i in range(nclc):
                clc[(16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)[i]] = get(3)
            cl, lens = table(clc), []
            while len(lens) < nlit + ndist:
                s = symbol(cl)
                lens += [s] if s < 16 else [lens[-1]] * (get(2) + 3) if s == 16 else [0] * (get(3) + 3) if s == 17 else [0] * (get(7) + 11)
            lit, dst = table(lens[:nlit]), table(lens[nlit:])
        while True:
            s = symbol(lit)
            if s < 256:
                out += 1
            elif s == 256:
                break
            else:
                n = LENGTH_BASE[s - 257] + get(LENGTH_EXTRA[s - 257])
                d = symbol(dst)
                d = DIST_BASE[d] + get(DIST_EXTRA[d])
                out, far, longest = out + n, max(far, d), max(longest, n)
    return out, far, longest


@functools.lru_cache(None)
def damage_cases():
    """(name, file, status)"""
    w, h, color = 20, 12, 2
    raw = image(w, h, color, seed=20)
    scan = filter_rows(raw, 3, [y % 5 for y in range(h)])
    z = deflate(scan, 6)
    zs = deflate(scan, 0)
    good = png(w, h, color, z)
    out = []

    def stream(name, s, status=INVALID_IDAT, **kw):
        out.append((name, png(w, h, color, s, **kw), status))

    stream("zlib_cm", bytes([0x79, 0x9C ^ 0]) + z[2:])
    stream("zlib_window", bytes([0x88, 0x1C]) + z[2:])  # CINFO 8, FCHECK right
    stream("zlib_fdict", bytes([0x78, 0xBB]) + z[2:])   # FDICT set, FCHECK right
    stream("zlib_fcheck", bytes([0x78, 0x9D]) + z[2:])
    stream("block_type_3", b"\x78\x9c" + _bits((1, 1), (3, 2)) + bytes(8))
    stream("stored_len_nlen", zs[:5] + bytes([zs[5] ^ 1]) + zs[6:])
    # dynamic headers: HLIT 0, HDIST 0, HCLEN 15 (all 19 code length code lengths)
    def dyn(clc, body):  # clc: lengths for symbols 0..18
        order = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
        return b"\x78\x9c" + _bits((1, 1), (2, 2), (0, 5), (0, 5), (15, 4), *[(clc[s], 3) for s in order], *body) + bytes(8)

    stream("clc_oversubscribed", dyn([1] * 19, []))
    stream("clc_incomplete", dyn([2, 2] + [0] * 17, []))
    # code length code: symbols 1 and 16 with 1 bit each -> codes 0 (a length of 1) and 1 (repeat)
    clc = [0] * 19
    clc[1], clc[16] = 1, 1
    stream("repeat_without_previous", dyn(clc, [(1, 1), (0, 2)]))
    # 258 lengths of 1: over-subscribed literal/length code
    stream("lit_oversubscribed", dyn(clc, [(0, 1)] + [(1, 1), (3, 2)] * 43))
    # symbols 0 and 8 -> 1 bit each: 257 lengths of 8 (256 codes would be complete) is over-subscribed; 0 then 8 ... use zeros to be incomplete
    clc2 = [0] * 19
    clc2[0], clc2[8] = 1, 1
    stream("lit_incomplete", dyn(clc2, [(1, 1)] * 100 + [(0, 1)] * 156 + [(1, 1)] + [(0, 1)]))
    stream("no_end_of_block_code", dyn(clc2, [(1, 1)] * 256 + [(0, 1)] + [(0, 1)]))
    # fixed blocks: symbol 286 = the 8-bit code 11000110 (sent MSB first), distance symbol 30 = 11110
    def msb(code, n):
        return (int(format(code, f"0{n}b")[::-1], 2), n)

    stream("fixed_symbol_286", b"\x78\x9c" + _bits((1, 1), (1, 2), msb(0b11000110, 8)) + bytes(8))
    stream("fixed_symbol_287", b"\x78\x9c" + _bits((1, 1), (1, 2), msb(0b11000111, 8)) + bytes(8))
    lit_a = msb(0x30 + 65, 8)
    len3 = msb(1, 7)  # symbol 257: length 3
    stream("fixed_distance_30", b"\x78\x9c" + _bits((1, 1), (1, 2), lit_a, len3, msb(30, 5)) + bytes(8))
    stream("fixed_distance_31", b"\x78\x9c" + _bits((1, 1), (1, 2), lit_a, len3, msb(31, 5)) + bytes(8))
    stream("distance_before_start", b"\x78\x9c" + _bits((1, 1), (1, 2), lit_a, len3, msb(1, 5)) + bytes(8))  # distance 2 after one byte
    stream("ends_before_eob", z[: len(z) // 2])
    stream("ends_before_eob_stored", zs[: len(zs) // 2])
    stream("too_little_output", deflate(scan[:-1], 6))
    bad_filter = bytearray(scan)
    bad_filter[(1 + w * 3) * 5] = 5
    stream("filter_byte_5", deflate(bytes(bad_filter), 6))
    plte = bytes(range(30))
    idx = np.full((4, 8), 3, np.uint8)
    idx[2, 5] = 10
    out.append(("palette_index_past_plte", png(8, 4, 3, deflate(filter_rows(idx, 1, [0] * 4)) + bytes(40), plte=plte), INVALID_IDAT))
    pz = deflate(filter_rows(np.zeros((4, 8), np.uint8), 1, [0] * 4)) + bytes(40)
    out.append(("palette_without_plte", png(8, 4, 3, pz), CHUNK_PARSING))
    out.append(("plte_not_multiple_of_3", png(8, 4, 3, pz, plte=bytes(31)), CHUNK_PARSING))
    out.append(("plte_too_long", png(8, 4, 3, pz, plte=bytes(771)), CHUNK_PARSING))
    # containers
    out.append(("chunk_leaves_file", good[:33] + struct.pack(">I", 5000) + good[37:], CHUNK_PARSING))
    out.append(("no_idat", SIG + good[8:33] + chunk(b"tEXt", bytes(60)) + chunk(b"IEND"), CHUNK_PARSING))
    out.append(("idat_not_consecutive", png(w, h, color, z, idat=[z[:40], z[40:]])[: 33 + 12 + 40] + chunk(b"tEXt", b"a\0b") + chunk(b"IDAT", z[40:]) + chunk(b"IEND"), CHUNK_PARSING))
    out.append(("idat_after_stream", png(w, h, color, z, after_idat=[chunk(b"tEXt", b"a\0b"), chunk(b"IDAT", b"")]), CHUNK_PARSING))
    out.append(("unknown_critical_chunk", png(w, h, color, z, before_plte=[chunk(b"ABcd", bytes(4))]), UNSUPPORTED))
    out.append(("unknown_critical_behind_idat", png(w, h, color, z, after_idat=[chunk(b"FRAm", bytes(30))]), UNSUPPORTED))
    out.append(("bad_signature", b"\x89PNX" + good[4:], NOT_PNG))
    out.append(("ihdr_crc", good[:29] + bytes([good[29] ^ 1]) + good[30:], HEADER_CRC32))
    out.append(("zero_width", png(0, h, color, z), BAD_DIMS))
    for depth, col in ((1, 0), (2, 3), (4, 0), (16, 2), (16, 6)):
        out.append((f"depth{depth}_color{col}", png(w, h, col, z, depth=depth, plte=bytes(48) if col == 3 else None), UNSUPPORTED))
    out.append(("adam7", png(w, h, color, z, interlace=1), UNSUPPORTED))
    return out


def sweep_sources():
    """the three 32 x 32 files of the truncation / byte-change sweeps"""
    plte = np.random.default_rng(30).integers(0, 256, 3 * 64, dtype=np.uint8).tobytes()
    return [("rgb_paeth", make(32, 32, 2, filters=4, seed=31)),
            ("palette_trns", make(32, 32, 3, seed=32, plte=plte, trns=bytes(range(40, 90)))),
            ("rgba_mixed", make(32, 32, 6, seed=33))]


def sweep_files(name, file, changes=2000, seed=1234):
    """every truncation length, then `changes` single-byte changes (a fixed seed)"""
    out = [(f"{name}_cut{n}", file[:n]) for n in range(len(file))]
    rng = np.random.default_rng(seed)
    for k in range(changes):
        at, val = int(rng.integers(8, len(file))), int(rng.integers(1, 256))
        out.append((f"{name}_chg{k}", file[:at] + bytes([file[at] ^ val]) + file[at + 1:]))
    return out
