"""Files with wrong checksums for the decode-verify tests (TEST INFRASTRUCTURE), and Python's zlib as their judge.

The edits keep the token stream in step -- one literal of a compressed file changed, one pixel byte of a stored file changed -- so
the decoder accepts the file with status 0 by default; what is wrong is the IDAT chunk's CRC-32, the zlib stream's Adler-32, or both.
zlib says which: crc_is_bad() holds zlib.crc32(b"IDAT" + payload) against the stored word, adler_is_bad() lets zlib inflate the
payload, which raises "incorrect data check" exactly when the Adler-32 is wrong."""
import ctypes as C
import struct
import zlib

import numpy as np

from token_mutator import Stream

LUT_WORDS = 4160


def plan(png):
    """fpng_amd_decode_plan: (result, mode, idat_ofs, idat_len, first_bit, limit_bit, lut) -- the host's view, no GPU"""
    from fpng_amd import _lib
    lib = _lib.load()
    b = np.frombuffer(bytes(png), dtype=np.uint8)
    res = _lib.DecodeResult()
    mode, ofs, ln = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    first, limit = C.c_uint64(0), C.c_uint64(0)
    lut = (C.c_uint32 * LUT_WORDS)()
    rc = lib.fpng_amd_decode_plan(b.ctypes.data, b.size, C.byref(res), C.byref(mode), C.byref(ofs), C.byref(ln), C.byref(first), C.byref(limit), C.byref(lut))
    assert rc == 0
    return res, mode.value, ofs.value, ln.value, first.value, limit.value, np.frombuffer(lut, dtype=np.uint32).copy()


def idat(png):
    """(offset of the IDAT chunk, payload length) by a chunk walk of its own"""
    ofs = 8
    while ofs + 12 <= len(png):
        (ln,) = struct.unpack(">I", png[ofs:ofs + 4])
        if png[ofs + 4:ofs + 8] == b"IDAT":
            return ofs, ln
        ofs += 12 + ln
    raise AssertionError("no IDAT")


def payload(png):
    ofs, ln = idat(png)
    return bytes(png[ofs + 8:ofs + 8 + ln])


def crc_is_bad(png):
    ofs, ln = idat(png)
    return zlib.crc32(b"IDAT" + bytes(png[ofs + 8:ofs + 8 + ln])) != struct.unpack(">I", png[ofs + 8 + ln:ofs + 12 + ln])[0]


def adler_is_bad(png):
    try:
        zlib.decompressobj().decompress(payload(png))
        return False
    except zlib.error as e:
        assert "incorrect data check" in str(e), e
        return True


def expected_status(png, knob):
    """what a file that decodes with status 0 by default returns with FPNG_AMD_VERIFY_* = knob, zlib being the judge"""
    if (knob & 1) and crc_is_bad(png):
        return 65
    if (knob & 2) and adler_is_bad(png):
        return 66
    return 0


def filtered_bytes(png):
    """the bytes the zlib stream stands for (the trailer is not looked at)"""
    return zlib.decompressobj(-15).decompress(payload(png)[2:])


def with_adler(png, adler, fix_crc=True):
    """the file with `adler` as the last four payload bytes; fix_crc: the chunk's CRC recomputed (else the old word stays)"""
    ofs, ln = idat(png)
    z = bytes(png[ofs + 8:ofs + 8 + ln - 4]) + struct.pack(">I", adler & 0xFFFFFFFF)
    crc = struct.pack(">I", zlib.crc32(b"IDAT" + z)) if fix_crc else bytes(png[ofs + 8 + ln:ofs + 12 + ln])
    return bytes(png[:ofs + 8]) + z + crc + bytes(png[ofs + 12 + ln:])


def stored_adler(png):
    ofs, ln = idat(png)
    return struct.unpack(">I", png[ofs + 4 + ln:ofs + 8 + ln])[0]


def flip_crc_bit(png, bit=5):
    ofs, ln = idat(png)
    b = bytearray(png)
    b[ofs + 8 + ln + bit // 8] ^= 1 << (bit % 8)
    return bytes(b)


def edit_literal(png, where, rng):
    """A compressed file with exactly ONE non-filter literal changed, the stream otherwise bit for bit (small files: the whole token list
    is rewritten).  where: 0..1, the place in the stream.  -> (file with the correct Adler-32 and CRC, the same with the ORIGINAL file's
    Adler-32 and a correct CRC, the same with the original Adler-32 and the original CRC word)"""
    s = Stream(png, plan)
    T = list(s.tokens)
    pos = s.positions(T)
    lits = [i for i, t in enumerate(T) if t[0] == "lit" and pos[i] % s.stride]
    assert lits
    i = lits[min(len(lits) - 1, int(where * len(lits)))]
    others = sorted(v for v in s.lit_code if v != T[i][1])
    T[i] = ("lit", others[int(rng.integers(0, len(others)))])
    out = s.write(T)
    assert out is not None
    good = with_adler(out, zlib.adler32(filtered_bytes(out)))
    stale = with_adler(out, stored_adler(png))
    ofs, ln = idat(png)
    o2, l2 = idat(stale)
    stale_crc = stale[:o2 + 8 + l2] + bytes(png[ofs + 8 + ln:ofs + 12 + ln]) + stale[o2 + 12 + l2:]
    return good, stale, stale_crc


def edit_literal_large(png, emul_lib, row, col_lo, col_hi, rng, stream=None):
    """The same for a LARGE file (token_mutator.LargeStream: one literal spliced): the edited literal is a data byte of output row
    `row` at byte col_lo <= column < col_hi of the row's data.  -> (stale Adler-32 with a correct CRC, stale Adler-32 with the
    original CRC word), or None when no literal lies there"""
    from token_mutator import LargeStream
    s = stream if stream is not None else LargeStream(png, plan, emul_lib)
    lo, hi = (int(np.searchsorted(s.out_pos, y * s.stride)) for y in (row, row + 1))
    hi = min(hi, s.n - 1)
    col = s.out_pos[lo:hi] % s.stride
    idx = np.flatnonzero((s.kind[lo:hi] == 0) & (col >= 1 + col_lo) & (col < 1 + col_hi))
    if not len(idx):
        return None
    j = lo + int(idx[int(rng.integers(0, len(idx)))])
    others = sorted(v for v in s.lit_code if v != int(s.value[j]))
    out = s.splice(j, j + 1, [("lit", others[int(rng.integers(0, len(others)))])])
    assert out is not None
    stale = with_adler(out, stored_adler(png))
    ofs, ln = idat(png)
    o2, l2 = idat(stale)
    return stale, stale[:o2 + 8 + l2] + bytes(png[ofs + 8 + ln:ofs + 12 + ln]) + stale[o2 + 12 + l2:]


def edit_stored_byte(png, w, h, c, y, xbyte, fix_crc=True):
    """A stored file with ONE pixel byte changed (row y, byte xbyte of the row's data): the Adler-32 is stale; fix_crc: the CRC recomputed"""
    ofs, ln = idat(png)
    s = y * (w * c + 1) + 1 + xbyte           # byte of the filtered stream
    p = 2 + 5 * (s // 65535 + 1) + s          # ... of the payload (blocks of 65535 bytes behind 5-byte headers)
    b = bytearray(png)
    b[ofs + 8 + p] ^= 0x5A
    if fix_crc:
        b[ofs + 8 + ln:ofs + 12 + ln] = struct.pack(">I", zlib.crc32(b"IDAT" + bytes(b[ofs + 8:ofs + 8 + ln])))
    return bytes(b)
