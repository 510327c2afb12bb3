"""ctypes doors into the CPU checkers (TEST INFRASTRUCTURE).

`oracle`  : oracle/libfpng_oracle.so  -- the row-local C restatement (always available; built by
            __graft_entry__.build() / `make -C oracle`).
`ref`     : oracle/_ref/libfpng_ref.so -- the UNMODIFIED reference, compiled by oracle/Makefile where its sources are
            at hand; elsewhere its recorded encode / decode answers (tests/golden/ref_answers.npz).
"""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_DIR = os.path.join(ROOT, "oracle")


def _ensure_built():
    so = os.path.join(ORACLE_DIR, "libfpng_oracle.so")
    src = os.path.join(ORACLE_DIR, "fpng_oracle.c")
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        subprocess.check_call(["make", "-C", ORACLE_DIR], stdout=subprocess.DEVNULL)


class _Oracle:
    def __init__(self):
        _ensure_built()
        L = C.CDLL(os.path.join(ORACLE_DIR, "libfpng_oracle.so"))
        L.fpo_crc32.restype = C.c_uint32
        L.fpo_crc32.argtypes = [C.c_void_p, C.c_size_t, C.c_uint32]
        L.fpo_adler32.restype = C.c_uint32
        L.fpo_adler32.argtypes = [C.c_void_p, C.c_size_t, C.c_uint32]
        L.fpo_max_encoded_size.restype = C.c_size_t
        L.fpo_max_encoded_size.argtypes = [C.c_uint32] * 3
        L.fpo_encode.restype = C.c_int
        L.fpo_encode.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t,
                                 C.POINTER(C.c_size_t)]
        L.fpo_encode_band_1pass.restype = C.c_uint64
        L.fpo_encode_band_1pass.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                            C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                            C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
        L.fpo_get_1pass_table.restype = None
        L.fpo_get_1pass_table.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p),
                                          C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.fpo_get_len_tables.restype = None
        L.fpo_get_len_tables.argtypes = [C.c_void_p, C.c_void_p]
        L.fpo_build_dynamic_table.restype = C.c_uint32
        L.fpo_build_dynamic_table.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.fpo_train_tables.restype = C.c_uint32
        L.fpo_train_tables.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        self.L = L

    def crc32(self, data, prev=0):
        b = np.ascontiguousarray(np.frombuffer(bytes(data), dtype=np.uint8)) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data)
        return self.L.fpo_crc32(b.ctypes.data, b.size, prev)

    def adler32(self, data, prev=1):
        b = np.ascontiguousarray(np.frombuffer(bytes(data), dtype=np.uint8)) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data)
        return self.L.fpo_adler32(b.ctypes.data, b.size, prev)

    def max_size(self, w, h, c):
        return self.L.fpo_max_encoded_size(w, h, c)

    def encode(self, img, w, h, c, flags=0):
        """img: uint8 array of w*h*c bytes -> PNG bytes (or None on bad args)."""
        img = np.ascontiguousarray(img, dtype=np.uint8)
        cap = self.max_size(w, h, c) if (w and h and c in (3, 4)) else 64
        out = np.zeros(cap, dtype=np.uint8)
        n = C.c_size_t(0)
        ok = self.L.fpo_encode(img.ctypes.data, w, h, c, flags, out.ctypes.data, cap, C.byref(n))
        return out[: n.value].tobytes() if ok else None

    def band_1pass(self, img, w, h, c, y0, y1):
        img = np.ascontiguousarray(img, dtype=np.uint8)
        cap = ((w * c + 1) * (y1 - y0) * 12 + 7) // 8 + 64
        out = np.zeros(cap, dtype=np.uint8)
        s1, s2, ln, lu = C.c_uint32(0), C.c_uint32(0), C.c_uint64(0), C.c_uint32(0)
        bits = self.L.fpo_encode_band_1pass(img.ctypes.data, w, h, c, y0, y1, out.ctypes.data, cap, C.byref(s1),
                                            C.byref(s2), C.byref(ln), C.byref(lu))
        self.last_unit_bits = lu.value
        return bits, out[: (bits + 7) // 8].copy(), s1.value, s2.value, ln.value

    def table_1pass(self, c):
        lens = np.zeros(288, dtype=np.uint8)
        codes = np.zeros(288, dtype=np.uint16)
        p = C.c_void_p()
        plen, sbit = C.c_uint32(0), C.c_uint32(0)
        self.L.fpo_get_1pass_table(c, lens.ctypes.data, codes.ctypes.data, C.byref(p), C.byref(plen), C.byref(sbit))
        prefix = C.string_at(p, plen.value)
        return lens, codes, prefix, sbit.value

    def len_tables(self):
        sym = np.zeros(256, dtype=np.uint16)
        ex = np.zeros(256, dtype=np.uint8)
        self.L.fpo_get_len_tables(sym.ctypes.data, ex.ctypes.data)
        return sym, ex

    def build_dynamic_table(self, hist, c):
        hist = np.ascontiguousarray(hist, dtype=np.uint32)
        lens = np.zeros(288, dtype=np.uint8)
        codes = np.zeros(288, dtype=np.uint16)
        hdr = np.zeros(400, dtype=np.uint8)
        bits = self.L.fpo_build_dynamic_table(hist.ctypes.data, c, lens.ctypes.data, codes.ctypes.data, hdr.ctypes.data)
        return lens, codes, hdr, bits


    def train_tables(self, imgs, c):
        """-> dict like tests/golden/train.json: prefix bytes (hex), pending bits, codes, code sizes."""
        imgs = [np.ascontiguousarray(i, dtype=np.uint8) for i in imgs]
        n = len(imgs)
        ptrs = (C.c_void_p * n)(*[i.ctypes.data for i in imgs])
        ws = (C.c_uint32 * n)(*[i.shape[1] for i in imgs])
        hs = (C.c_uint32 * n)(*[i.shape[0] for i in imgs])
        lens = np.zeros(288, dtype=np.uint8)
        codes = np.zeros(288, dtype=np.uint16)
        hdr = np.zeros(400, dtype=np.uint8)
        bits = self.L.fpo_train_tables(ptrs, ws, hs, n, c, lens.ctypes.data, codes.ctypes.data, hdr.ctypes.data)
        return table_record(hdr, bits, codes, lens)


def table_record(hdr, bits, codes, lens):
    """Header bytes + bit count of a block prefix in the form the reference's training mode prints it (src/fpng_test.cpp:905-925):
    whole bytes, then the pending bits."""
    nb = bits // 8
    return {"prefix": bytes(hdr[:nb]).hex(), "bit_buf": int(hdr[nb]) & ((1 << (bits % 8)) - 1), "bit_buf_size": bits % 8,
            "codes": [int(v) for v in codes], "code_sizes": [int(v) for v in lens]}


class _Ref:
    def __init__(self):
        path = os.path.join(ORACLE_DIR, "_ref", "libfpng_ref.so")
        if not os.path.exists(path):
            _ensure_built()
        if not os.path.exists(path):
            raise FileNotFoundError(path)
        L = C.CDLL(path)
        L.ref_init.restype = None
        L.ref_supports_sse41.restype = C.c_int
        L.ref_crc32.restype = C.c_uint32
        L.ref_crc32.argtypes = [C.c_void_p, C.c_size_t, C.c_uint32]
        L.ref_adler32.restype = C.c_uint32
        L.ref_adler32.argtypes = [C.c_void_p, C.c_size_t, C.c_uint32]
        L.ref_encode.restype = C.c_int
        L.ref_encode.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t,
                                 C.POINTER(C.c_size_t)]
        L.ref_get_info.restype = C.c_int
        L.ref_get_info.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                   C.POINTER(C.c_uint32)]
        L.ref_decode.restype = C.c_int
        L.ref_decode.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32),
                                 C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_uint32]
        L.ref_time_encode.restype = C.c_double
        L.ref_time_encode.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int,
                                      C.POINTER(C.c_size_t)]
        if hasattr(L, "ref_time_decode"):
            L.ref_time_decode.restype = C.c_double
            L.ref_time_decode.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int]
        L.ref_init()
        self.L = L

    def crc32(self, data, prev=0):
        b = np.ascontiguousarray(data, dtype=np.uint8)
        return self.L.ref_crc32(b.ctypes.data, b.size, prev)

    def adler32(self, data, prev=1):
        b = np.ascontiguousarray(data, dtype=np.uint8)
        return self.L.ref_adler32(b.ctypes.data, b.size, prev)

    def encode(self, img, w, h, c, flags=0):
        img = np.ascontiguousarray(img, dtype=np.uint8)
        n_f = (w * c + 1) * h
        cap = 58 + 6 + n_f + 5 * ((n_f + 65534) // 65535) + 16 + 64
        out = np.zeros(cap, dtype=np.uint8)
        n = C.c_size_t(0)
        ok = self.L.ref_encode(img.ctypes.data, w, h, c, flags, out.ctypes.data, cap, C.byref(n))
        return out[: n.value].tobytes() if ok else None

    def get_info(self, png):
        """fpng_get_info -> (status, w, h, c)"""
        b = np.frombuffer(bytes(png), dtype=np.uint8)
        w, h, c = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        st = self.L.ref_get_info(b.ctypes.data, b.size, C.byref(w), C.byref(h), C.byref(c))
        return st, w.value, h.value, c.value

    def decode(self, png, desired):
        b = np.frombuffer(png, dtype=np.uint8)
        w, h, c = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        st = self.L.ref_get_info(b.ctypes.data, b.size, C.byref(w), C.byref(h), C.byref(c))
        if st != 0:
            return st, None, 0, 0, 0
        out = np.zeros(w.value * h.value * desired, dtype=np.uint8)
        st = self.L.ref_decode(b.ctypes.data, b.size, out.ctypes.data, out.size, C.byref(w), C.byref(h), C.byref(c),
                               desired)
        return st, out, w.value, h.value, c.value

    def time_decode(self, png, desired, reps=3):
        """best seconds of `reps` fpng_decode_memory() calls into one reused vector (the reference harness's way)"""
        b = np.frombuffer(png, dtype=np.uint8)
        secs = self.L.ref_time_decode(b.ctypes.data, b.size, desired, reps)
        assert secs > 0, f"reference decoder status {-secs}"
        return secs

    def time_encode(self, img, w, h, c, flags=0, reps=3):
        img = np.ascontiguousarray(img, dtype=np.uint8)
        n = C.c_size_t(0)
        return self.L.ref_time_encode(img.ctypes.data, w, h, c, flags, reps, C.byref(n)), n.value


_oracle = None
_ref = None


def oracle():
    global _oracle
    if _oracle is None:
        _oracle = _Oracle()
    return _oracle


def have_ref():
    """The reference build itself (oracle/_ref, made by build() where the reference's sources are at hand)."""
    return os.path.exists(os.path.join(ORACLE_DIR, "_ref", "libfpng_ref.so"))


ANSWERS = os.path.join(ROOT, "tests", "golden", "ref_answers.npz")


def have_ref_answers():
    """ref().encode / ref().decode can be answered: by the reference build, or else by its recorded answers."""
    return have_ref() or os.path.exists(ANSWERS)


def ref():
    global _ref
    if _ref is None:
        if os.environ.get("FPNG_RECORD_REF_ANSWERS"):
            _ref = _RecordingRef(_Ref())
        elif have_ref():
            _ref = _Ref()
        else:
            _ref = _RecordedRef()
    return _ref


# ---------------------------------------------------------------------------------------------
# The reference's answers, recorded (tests/golden/ref_answers.npz, oracle/make_golden_ref_answers.py)
# ---------------------------------------------------------------------------------------------
def _digest(*parts):
    import hashlib
    h = hashlib.blake2b(digest_size=16)
    for p in parts:
        h.update(p if isinstance(p, (bytes, bytearray, memoryview)) else np.ascontiguousarray(p).tobytes())
    return h.digest()


def _encode_key(img, w, h, c, flags):
    return _digest(b"E", np.array([w, h, c, flags], dtype=np.int64), np.ascontiguousarray(img, dtype=np.uint8))


def _decode_key(png, desired):
    return _digest(b"D", np.array([desired], dtype=np.int64), bytes(png))


def _info_key(png):
    return _digest(b"I", bytes(png))


class _RecordingRef:
    """FPNG_RECORD_REF_ANSWERS=1: the reference answers, and every encode / decode call's answer is kept (size or status and
    dimensions, a digest of the bytes) and merged into tests/golden/ref_answers.npz when the process ends."""

    def __init__(self, real):
        import atexit
        self.real, self.L, self.rows = real, real.L, {}
        atexit.register(self.save)

    def encode(self, img, w, h, c, flags=0):
        png = self.real.encode(img, w, h, c, flags)
        self.rows[_encode_key(img, w, h, c, flags)] = ((-1, 0, 0, 0), b"\0" * 16) if png is None else ((len(png), 0, 0, 0), _digest(png))
        return png

    def get_info(self, png):
        info = self.real.get_info(png)
        self.rows[_info_key(png)] = (info, b"\0" * 16)
        return info

    def decode(self, png, desired):
        st, out, w, h, c = self.real.decode(png, desired)
        self.rows[_decode_key(png, desired)] = ((st, w, h, c), _digest(out) if st == 0 else b"\0" * 16)
        return st, out, w, h, c

    def __getattr__(self, name):
        return getattr(self.real, name)

    def save(self):
        rows = dict(_load_answers()) if os.path.exists(ANSWERS) else {}
        rows.update(self.rows)
        keys = sorted(rows)
        np.savez_compressed(ANSWERS, keys=np.frombuffer(b"".join(keys), np.uint8).reshape(-1, 16),
                            ints=np.array([rows[k][0] for k in keys], dtype=np.int64).reshape(-1, 4),
                            digests=np.frombuffer(b"".join(rows[k][1] for k in keys), np.uint8).reshape(-1, 16))


def _load_answers():
    z = np.load(ANSWERS)
    return {bytes(k): (tuple(int(v) for v in i), bytes(d)) for k, i, d in zip(z["keys"], z["ints"], z["digests"])}


class _RecordedRef:
    """The reference's recorded answers, for a checkout without the reference build.  The bytes handed back are computed here
    -- the file by the C restatement (oracle/), the pixels by the drop-in's CPU decoder -- and must have the digest the
    reference's own bytes had: a call whose answer was never recorded, or bytes that differ from the reference's, fail."""

    def __init__(self):
        self.rows = _load_answers()

    def _row(self, key, what):
        if key not in self.rows:
            raise AssertionError(f"no recorded reference answer for this {what} call (oracle/make_golden_ref_answers.py records them)")
        return self.rows[key]

    def encode(self, img, w, h, c, flags=0):
        (size, *_), dig = self._row(_encode_key(img, w, h, c, flags), "encode")
        if size < 0:
            return None
        png = oracle().encode(img, w, h, c, flags)
        assert png is not None and len(png) == size and _digest(png) == dig, "the C restatement's file differs from the reference's"
        return png

    def get_info(self, png):
        return self._row(_info_key(png), "get_info")[0]

    def decode(self, png, desired):
        (st, w, h, c), dig = self._row(_decode_key(png, desired), "decode")
        if st != 0:
            return st, None, w, h, c
        import dropin
        old = os.environ.get("FPNG_AMD_DECODE_CPU")
        os.environ["FPNG_AMD_DECODE_CPU"] = "1"
        try:
            st2, out, *_ = dropin.decode(png, desired)
        finally:
            if old is None:
                del os.environ["FPNG_AMD_DECODE_CPU"]
            else:
                os.environ["FPNG_AMD_DECODE_CPU"] = old
        assert st2 == 0 and _digest(np.asarray(out)) == dig, "the drop-in's pixels differ from the reference's"
        return st, np.asarray(out), w, h, c


# ---------------------------------------------------------------------------------------------
# Fuzz image recipe that actually reaches the edge cases
# ---------------------------------------------------------------------------------------------
def fuzz_image(rng, force_dims=None, c=None):
    """Returns (img uint8[h,w,c], w, h, c): random runs / vertical copies / deltas / noise."""
    if c is None:
        c = int(rng.integers(3, 5))
    if force_dims is not None:
        w, h = force_dims
    else:
        u = rng.random()
        if u < 0.15:
            w, h = int(rng.integers(1, 7)), int(rng.integers(1, 7))
        elif u < 0.30:
            w, h = int(rng.integers(60, 401)), int(rng.integers(1, 5))
        else:
            w, h = int(rng.integers(1, 49)), int(rng.integers(1, 15))
    q = rng.random() ** 2
    p_run = rng.random() * 0.7
    p_up = rng.random() * 0.5
    amp = int(rng.choice([1, 2, 4, 16, 256]))
    img = np.zeros((h, w, c), dtype=np.uint8)
    r = rng.random((h, w, 3))
    noise = rng.integers(0, 256, size=(h, w, c), dtype=np.int64)
    delta = rng.integers(0, amp, size=(h, w, c), dtype=np.int64) if amp > 1 else np.zeros((h, w, c), dtype=np.int64)
    for y in range(h):
        for x in range(w):
            if r[y, x, 0] < q:
                img[y, x] = noise[y, x]
            elif x > 0 and r[y, x, 1] < p_run:
                # copy-left in FILTERED space: pixel - up == left - left_up
                if y > 0:
                    img[y, x] = (img[y, x - 1].astype(np.int64) - img[y - 1, x - 1] + img[y - 1, x]) & 0xFF
                else:
                    img[y, x] = img[y, x - 1]
            elif y > 0 and r[y, x, 2] < p_up:
                img[y, x] = img[y - 1, x]
            else:
                base = img[y - 1, x].astype(np.int64) if y > 0 else np.zeros(c, dtype=np.int64)
                img[y, x] = (base + delta[y, x]) & 0xFF
    return img, w, h, c
