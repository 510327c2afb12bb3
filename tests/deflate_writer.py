"""A deflate / zlib writer driven by tokens, for the general decode tier's tests (inflate_cases.py): the caller says which blocks a
stream has, which tokens each holds, with which code lengths and which sequence of code-length symbols the codes are sent, and
gets the stream, the bytes it means and a log of what it contains.  Nothing here reads a decoder: the log is the writer's own
account, so a test can assert what a corpus covers without asking the code under test.

    stream, data, log = write([stored(b"..."), fixed([0, 65, (3, 1)]), dynamic(tokens, lit_lens, dist_lens, cl_syms, clc_lens)])

A token is a literal (an int), a match (length, distance) or (length, distance, length symbol) -- 258 may be sent as symbol 284 with
extra 31 -- or, for streams that are meant to be refused, raw(value, width): bits as they are; a match's distance may be such bits
too.  The final block is the last one."""
import math
import struct
import zlib

LENGTH_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LENGTH_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
FIXED_LIT = (8,) * 144 + (9,) * 112 + (7,) * 24 + (8,) * 8
FIXED_DIST = (5,) * 32


def _bits(*fields):
    """(value, width) fields, LSB first -> bytes (short hand-made pieces; streams go through BitWriter)"""
    v = at = 0
    for val, n in fields:
        v |= val << at
        at += n
    return v.to_bytes((at + 7) // 8, "little")


def _msb(code, n):
    """a Huffman code of n bits as a (value, width) field (codes go out most significant bit first)"""
    return (int(format(code, f"0{n}b")[::-1], 2), n)


class BitWriter:
    """LSB-first bits into a bytearray, a byte at a time"""

    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, val, width):
        self.acc |= (val & ((1 << width) - 1)) << self.n
        self.n += width
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def align(self):
        if self.n:
            self.out.append(self.acc)
            self.acc = self.n = 0

    def extend(self, data):
        assert self.n == 0
        self.out += data

    @property
    def pos(self):
        return 8 * len(self.out) + self.n

    def done(self):
        self.align()
        return bytes(self.out)


def canonical(lens):
    """code lengths -> {symbol: (the code as a field, bits reversed; its length)} (RFC 1951, 3.2.2)"""
    count = [0] * 17
    for ln in lens:
        count[ln] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for ln in range(1, 16):
        code = (code + count[ln - 1]) << 1
        nxt[ln] = code
    out = {}
    for s, ln in enumerate(lens):
        if ln:
            out[s] = _msb(nxt[ln] & ((1 << ln) - 1), ln)
            nxt[ln] += 1
    return out


def length_symbol(length):
    return 285 if length == 258 else 257 + max(k for k in range(28) if LENGTH_BASE[k] <= length)


def dist_symbol(dist):
    return max(k for k in range(30) if DIST_BASE[k] <= dist)


def kraft(lens):
    """the code space the lengths take, in units of 2^-15: 32768 is a complete code"""
    return sum(1 << (15 - ln) for ln in lens if ln)


def fill_code(assign, n, max_len=15, fillers=None):
    """lengths for n symbols: `assign` ({symbol: length}) as given, and as many of the other symbols (`fillers`, or ascending) as it
    takes to make the code complete"""
    rest = (1 << max_len) - sum(1 << (max_len - ln) for ln in assign.values())
    assert rest >= 0
    lens = [0] * n
    for s, ln in assign.items():
        lens[s] = ln
    free = list(fillers) if fillers is not None else [s for s in range(n) if s not in assign]
    for bit in range(max_len - 1, -1, -1):
        if (rest >> bit) & 1:
            lens[free.pop(0)] = max_len - bit
    assert assign and sum(1 << (max_len - ln) for ln in lens if ln) == 1 << max_len  # complete
    return lens


def flat_code(symbols, n):
    """a complete code over the symbols with two neighbouring lengths; one symbol alone gets the single 1-bit code"""
    symbols = sorted(set(symbols))
    lens, k = [0] * n, len(symbols)
    if k == 1:
        lens[symbols[0]] = 1
        return lens
    p = int(math.log2(k))
    r = k - (1 << p)
    for i, s in enumerate(symbols):
        lens[s] = p + 1 if i < 2 * r else p
    return lens


def random_code(symbols, max_len, rng, n, deep=0.3):
    """a random complete prefix code over the symbols (lengths for n symbols), no code longer than max_len: leaves of a binary
    tree are split until there is one per symbol -- with probability `deep` the deepest one that may still be split, else any.
    One symbol alone gets the single 1-bit code.  rng: a random.Random"""
    symbols = sorted(set(symbols))
    k = len(symbols)
    assert 1 <= k <= (1 << max_len)
    lens = [0] * n
    if k == 1:
        lens[symbols[0]] = 1
        return lens
    leaves = [1, 1]
    while len(leaves) < k:
        if rng.random() < deep:
            d = max((x for x in leaves if x < max_len), default=None)
            i = leaves.index(d) if d is not None else None
        else:
            i = rng.randrange(len(leaves))
            if leaves[i] >= max_len:
                i = None
        if i is None:
            i = min(range(len(leaves)), key=lambda j: leaves[j])  # (the shallowest can always be split while leaves are missing)
        d = leaves.pop(i)
        leaves += [d + 1, d + 1]
    rng.shuffle(leaves)
    for s, ln in zip(symbols, leaves):
        lens[s] = ln
    assert kraft(lens) == 32768 and max(lens) <= max_len
    return lens


def random_cl(lens, rng, repeats=0.7):
    """the code lengths as a sequence of code-length symbols: plain lengths and, where runs allow and the dice say so, (16, n),
    (17, n), (18, n) with a random n inside the run.  The lengths of both tables go in as one list, so a repeat may cross from one
    into the other, as RFC 1951 allows."""
    out, i = [], 0
    while i < len(lens):
        run = 1
        while i + run < len(lens) and lens[i + run] == lens[i]:
            run += 1
        if lens[i] == 0 and run >= 3 and rng.random() < repeats:
            if run >= 11 and rng.random() < 0.7:
                n = rng.choice((11, min(run, 138), rng.randint(11, min(run, 138))))
                out.append((18, n))
            else:
                n = rng.choice((3, min(run, 10), rng.randint(3, min(run, 10))))
                out.append((17, n))
            i += n
            continue
        if i and lens[i] == lens[i - 1] and rng.random() < repeats:
            back = 0  # (this run may have begun at i: count what lies at and behind i)
            while i + back < len(lens) and lens[i + back] == lens[i - 1]:
                back += 1
            if back >= 3:
                n = rng.choice((3, min(back, 6), rng.randint(3, min(back, 6))))
                out.append((16, n))
                i += n
                continue
        out.append(lens[i])
        i += 1
    return out


def expand_cl(cl_syms):
    """the lengths a sequence of code-length symbols stands for"""
    out = []
    for t in cl_syms:
        if isinstance(t, tuple):
            out += [out[-1] if t[0] == 16 else 0] * t[1]
        else:
            out.append(t)
    return out


def raw(value, width):
    return ("raw", value, width)


def stored(data, len_field=None):
    """len_field: a LEN other than the data's (for streams that are to be refused)"""
    return {"kind": "stored", "data": bytes(data), "len_field": len_field}


def fixed(tokens, eob=True):
    return {"kind": "fixed", "tokens": list(tokens), "eob": eob}


def dynamic(tokens, lit_lens=None, dist_lens=None, cl_syms=None, clc_lens=None, hclen=None, hlit=None, hdist=None, eob=True, check=True):
    """lit_lens: 257 .. 286 lengths (HLIT from their number), dist_lens: 1 .. 30; cl_syms: the code-length symbols that send them, a
    length or (16 | 17 | 18, repeat count) each (default: every length plainly); clc_lens: the code length code's 19 lengths
    (default: a flat code over the symbols cl_syms uses); hclen: how many of them are sent, 4 .. 19 (default: as few as possible).
    Codes left out are flat ones over what the tokens use.  hlit / hdist: header fields other than the lengths' numbers, and
    check=False: no insistence on a stream that holds together -- both for streams that are to be refused."""
    tokens = list(tokens)
    if lit_lens is None:
        lit_lens = flat_code({256} | {t for t in tokens if isinstance(t, int)} | {_length_symbol_of(t) for t in tokens if _is_match(t)}, 286)
        while len(lit_lens) > 257 and not lit_lens[-1]:
            lit_lens.pop()
    if dist_lens is None:
        used = {dist_symbol(t[1]) for t in tokens if _is_match(t) and isinstance(t[1], int)}
        dist_lens = flat_code(used, max(used) + 1) if used else [0]
    return {"kind": "dynamic", "tokens": tokens, "lit_lens": list(lit_lens), "dist_lens": list(dist_lens), "cl_syms": cl_syms, "clc_lens": clc_lens,
            "hclen": hclen, "hlit": hlit, "hdist": hdist, "eob": eob, "check": check}


def _is_match(t):
    return isinstance(t, tuple) and t[0] != "raw"


def _length_symbol_of(t):
    return t[2] if len(t) > 2 else length_symbol(t[0])


def zlib_header(cinfo=7):
    """CMF and FLG for a window of 2^(cinfo + 8) bytes, no dictionary, FCHECK right"""
    cmf = 8 | (cinfo << 4)
    return bytes([cmf, (31 - (cmf << 8) % 31) % 31])


def write(blocks, cinfo=7, adler=True, pad=0):
    """-> (the zlib stream, the bytes it means, the log).  pad: zero bytes behind the last block in place of nothing.
    log: {"blocks": [per block: kind, tokens (their number), out_start, out_end, end_bit (the bit of the deflate data, counted from
    its first byte, at which the block ends), and for Huffman blocks lit_used / dist_used (lengths of the codes the tokens were
    sent with), for dynamic ones lit_lens, dist_lens, lit_codes, dist_codes (how many symbols have a code), cl_used (lengths of the
    code-length codes sent), hlit, hdist, hclen, rep16_crosses (a symbol 16 whose run begins in the literal/length lengths and
    ends in the distance lengths), ends_with_repeat (16, 17, 18 or None: the repeat that ends exactly at HLIT + HDIST + 258)],
    "length_symbols" / "dist_symbols": {(symbol, extra value)}, "matches": [(length, distance, output position, block, token index)]}"""
    w, out = BitWriter(), bytearray()
    log = {"blocks": [], "length_symbols": set(), "dist_symbols": set(), "matches": []}
    for bi, b in enumerate(blocks):
        e = {"kind": b["kind"], "out_start": len(out), "tokens": 0}
        w.put(1 if bi == len(blocks) - 1 else 0, 1)
        if b["kind"] == "stored":
            n = len(b["data"]) if b["len_field"] is None else b["len_field"]
            w.put(0, 2)
            w.align()
            w.put(n, 16)
            w.put(~n & 0xFFFF, 16)
            w.extend(b["data"])
            out += b["data"]
        else:
            if b["kind"] == "fixed":
                w.put(1, 2)
                lit_lens, dist_lens = FIXED_LIT, FIXED_DIST
            else:
                w.put(2, 2)
                lit_lens, dist_lens = b["lit_lens"], b["dist_lens"]
                _dynamic_header(w, b, e)
            lit, dist = canonical(lit_lens), canonical(dist_lens)
            e["lit_used"], e["dist_used"] = set(), set()
            for ti, t in enumerate(b["tokens"]):
                if isinstance(t, int):
                    w.put(*lit[t])
                    e["lit_used"].add(lit[t][1])
                    out.append(t)
                elif t[0] == "raw":
                    w.put(t[1], t[2])
                    continue
                else:
                    length, d = t[0], t[1]
                    ls = _length_symbol_of(t)
                    extra = length - LENGTH_BASE[ls - 257]
                    assert 0 <= extra < (1 << LENGTH_EXTRA[ls - 257]) and 3 <= length <= 258, t
                    w.put(*lit[ls])
                    e["lit_used"].add(lit[ls][1])
                    w.put(extra, LENGTH_EXTRA[ls - 257])
                    log["length_symbols"].add((ls, extra))
                    if isinstance(d, tuple):  # raw bits in a distance's place: what they mean is the decoder's business
                        w.put(d[1], d[2])
                        continue
                    ds = dist_symbol(d)
                    w.put(*dist[ds])
                    e["dist_used"].add(dist[ds][1])
                    w.put(d - DIST_BASE[ds], DIST_EXTRA[ds])
                    log["dist_symbols"].add((ds, d - DIST_BASE[ds]))
                    log["matches"].append((length, d, len(out), bi, ti))
                    at = len(out) - d
                    for k in range(length):  # (in front of the output: zeros; such a stream is one to be refused)
                        out.append(out[at + k] if at + k >= 0 else 0)
                e["tokens"] += 1
            if b["eob"]:
                w.put(*lit[256])
                e["lit_used"].add(lit[256][1])
        e["end_bit"], e["out_end"] = w.pos, len(out)
        log["blocks"].append(e)
    body = w.done() + bytes(pad)
    return zlib_header(cinfo) + body + (struct.pack(">I", zlib.adler32(bytes(out))) if adler else b""), bytes(out), log


def _dynamic_header(w, b, e):
    lit_lens, dist_lens = b["lit_lens"], b["dist_lens"]
    cl_syms = b["cl_syms"] if b["cl_syms"] is not None else list(lit_lens) + list(dist_lens)
    used = {t[0] if isinstance(t, tuple) else t for t in cl_syms}
    clc = b["clc_lens"]
    if clc is None:
        clc = flat_code(used if len(used) > 1 else used | {min({0, 1} - used)}, 19)  # (the code length code must be complete)
    need = max([i + 1 for i, s in enumerate(CL_ORDER) if clc[s]] + [4])
    hclen = need if b["hclen"] is None else b["hclen"]
    hlit = len(lit_lens) - 257 if b["hlit"] is None else b["hlit"]
    hdist = len(dist_lens) - 1 if b["hdist"] is None else b["hdist"]
    if b["check"]:
        assert 257 <= len(lit_lens) <= 286 and 1 <= len(dist_lens) <= 30 and need <= hclen <= 19
        assert expand_cl(cl_syms) == list(lit_lens) + list(dist_lens), "the code-length symbols do not spell the lengths"
    w.put(hlit, 5)
    w.put(hdist, 5)
    w.put(hclen - 4, 4)
    for s in CL_ORDER[:hclen]:
        w.put(clc[s], 3)
    code = canonical(clc)
    cur, crosses, last = 0, False, None
    e["cl_used"] = set()
    for t in cl_syms:
        s, n = t if isinstance(t, tuple) else (t, 1)
        w.put(*code[s])
        e["cl_used"].add(code[s][1])
        if s >= 16:
            base, width = {16: (3, 2), 17: (3, 3), 18: (11, 7)}[s]
            assert 0 <= n - base < (1 << width), t
            w.put(n - base, width)
            crosses |= s == 16 and cur < len(lit_lens) < cur + n
        cur += n
        last = s if s >= 16 else None
    e.update(lit_lens=list(lit_lens), dist_lens=list(dist_lens), lit_codes=sum(1 for x in lit_lens if x), dist_codes=sum(1 for x in dist_lens if x),
             hlit=hlit, hdist=hdist, hclen=hclen, rep16_crosses=crosses, ends_with_repeat=last if cur == len(lit_lens) + len(dist_lens) else None)
