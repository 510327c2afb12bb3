"""Streams built to the edges of the GPU decoder's synchronisation (TEST INFRASTRUCTURE): dec_sync_kernel, dec_chain_kernel,
dec_offsets_kernel and dec_subscan_kernel of fpng_amd/csrc/decode.hip.

Every case is a VALID fpng-style file, small, built deterministically from content that is at hand and a seed that a search found
(kept here).  A case names the properties it was built for; `Trace` -- tests/cpp/decode_emul.cpp's fpng_emul_decode_trace, the
kernels' per-thread code run on the CPU with the kernels' constants -- says which branch of the synchronisation each block of the
file takes, and the predicates of `PROPS` hold the case to its name (tests/test_sync_cases_cpu.py).  The GPU then has to decode the
same files to the reference decoder's pixels (tests/test_gpu_decode_sync_geometry.py).

The geometry (decode_api.cpp make_job, decode.hip):
  * first_bit: the first row token's bit in the zlib stream; end_limit = 8 * (idat_len - 4); n_sub = ceil((end_limit - first_bit) / 512)
  * a workgroup takes 512 subsequences; the end-of-block code begins E bits behind first_bit and has L bits
  * the stream ends in the byte the code ends in (eob_status): end_limit - 7 <= first_bit + E + L <= end_limit.  So the file's last
    subsequence holds only PADDING bits exactly when the code ends on a subsequence border that is no byte border of the stream,
    i.e. (E + L) % 512 == 0 and first_bit % 8 != 0; with first_bit % 8 == 0 that subsequence does not exist (n_sub is 512, not 513).

Moving a stream's end by single bits: non-filter literals of the last rows are swapped for byte values whose code in the same table
is longer or shorter (`retimed`); the file stays a valid image -- other pixels."""
import ctypes as C
import functools

import numpy as np

import token_mutator as TM
from cpu_ref import oracle

SUB, BLOCK, LEAD_IN = 512, 512, 128   # bits of a subsequence, subsequences of a workgroup, bits of lead-in (decode.h)
GATHER_MIN, WAVE = 4, 64              # decode.hip: kGatherMin, kWave
MAX_WALKS_PER_ROW = 64                # decode.hip: kMaxWalksPerRow
MAX_CODE_BITS = 12                    # png_parse.h: kTableBits -- a file with a longer code is refused by the host's table check
MATCH_BITS_MAX = MAX_CODE_BITS + 5 + 1  # a length code, its extra bits, the distance bit

# ---- group D's bounds, derived --------------------------------------------------------------------------------------------------
# A subsequence decodes the tokens that BEGIN in [start, nominal + 512); its start lies at most MATCH_BITS_MAX - 1 bits behind its
# nominal first bit (the longest token that begins in front of it).  A literal puts out one byte for at most 12 bits; a match puts
# out three bytes and more for at most 13 (length 3 .. 10: no extra bits) and eleven and more for at most 18: literals of 12 bits
# are the fewest bytes per bit.  So a subsequence that is neither the file's first nor its last puts out at least
MIN_SUB_BYTES = -(-(SUB - (MATCH_BITS_MAX - 1)) // MAX_CODE_BITS)  # ceil(495 / 12) = 42


def max_walks(c):
    """The most walks of a window of 256 pixels of c bytes: the subsequences from the one the window's first byte lies in to the one
    the NEXT window's first byte lies in -- n = 256 * c + 2 bytes in a row for the first window of a row (its filter byte in front)
    -- of which all but the first and the last put out MIN_SUB_BYTES at least: 2 + (n - 2) // 42 = 26 (c = 4), 20 (c = 3)."""
    return 2 + (256 * c + 2 - 2) // MIN_SUB_BYTES


_TR_FILE, _TR_STEP, _TR_BLOCK, _TR_END, _TR_WALKS = 1, 2, 3, 4, 5
KIND_REDO, KIND_MAPS, KIND_LEFT = 0, 1, 2
LEFT_CRAWLING = 2


def _dm():
    import test_decode_model
    return test_decode_model


class Trace:
    """what fpng_emul_decode_trace says of a file (the records of tests/cpp/decode_emul.cpp)"""

    def __init__(self, png, desired=4):
        dm = _dm()
        L = dm.emul()
        u32p = C.POINTER(C.c_uint32)
        L.fpng_emul_decode_trace.restype = C.c_int
        L.fpng_emul_decode_trace.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, u32p, u32p, u32p, C.c_uint32, C.c_uint32, C.c_uint32, u32p,
                                             C.c_void_p, C.c_uint32, u32p]
        import dropin
        b = np.frombuffer(bytes(png), dtype=np.uint8)
        st, ww, hh, _ = dropin.get_info(png)
        assert st == 0
        out = np.zeros(ww * hh * desired + 16, dtype=np.uint8)
        w, h, c, n = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        stats = (C.c_uint32 * 4)()
        cap = 1 << 16
        while True:
            tr = np.zeros(cap, dtype=np.uint32)
            st = L.fpng_emul_decode_trace(b.ctypes.data, b.size, desired, out.ctypes.data, out.size, C.byref(w), C.byref(h), C.byref(c), BLOCK, LEAD_IN, 1000, stats,
                                          tr.ctypes.data, cap, C.byref(n))
            if st != -1010:
                break
            cap = n.value
        assert st > -1000, f"emulator internal error {st}"
        self.status, self.w, self.h, self.c = st, w.value, h.value, c.value
        self.pixels = out[: ww * hh * desired] if st == 0 else None
        self.steps, self.blocks, self.end, self.max_walks, self.min_bytes, self.n_sub = [], [], None, None, None, 0  # (a stored file has no records)
        v, i = [int(x) for x in tr[: n.value]], 0
        while i < len(v):
            tag = v[i]
            if tag == _TR_FILE:
                self.first_bit, self.end_limit, self.n_sub, self.eob_bits = v[i + 1] | v[i + 2] << 32, v[i + 3] | v[i + 4] << 32, v[i + 5], v[i + 6]
                i += 7
            elif tag == _TR_STEP:
                nt = v[i + 7]
                self.steps.append(dict(round=v[i + 1], blk=v[i + 2], valid=v[i + 3], it=v[i + 4], n_need=v[i + 5], kind=v[i + 6], threads=v[i + 8: i + 8 + nt]))
                i += 8 + nt
            elif tag == _TR_BLOCK:
                self.blocks.append(dict(round=v[i + 1], blk=v[i + 2], valid=v[i + 3], steps=v[i + 4], left=v[i + 5], maps=v[i + 6]))
                i += 7
            elif tag == _TR_END:
                self.end = (v[i + 1], v[i + 2])
                i += 3
            elif tag == _TR_WALKS:
                self.max_walks, self.min_bytes = v[i + 1], v[i + 2]
                i += 3
            else:
                raise AssertionError(f"unknown trace record {tag}")

    # the end-of-block code: its first bit behind first_bit, and its length
    @property
    def E(self):
        return self.end[0] * SUB + self.end[1] - self.eob_bits

    @property
    def L(self):
        return self.eob_bits

    def need(self, blk, rnd=0):
        """n_need of every step of block `blk` in round `rnd` that decoded threads again ([]: none was needed; None: not open)"""
        if not any(b["round"] == rnd and b["blk"] == blk for b in self.blocks):
            return None
        return [s["n_need"] for s in self.steps if s["round"] == rnd and s["blk"] == blk and s["kind"] != KIND_LEFT]

    def block(self, blk, rnd=0):
        return next((b for b in self.blocks if b["round"] == rnd and b["blk"] == blk), None)

    def step(self, blk, it, rnd=0):
        return next((s for s in self.steps if s["round"] == rnd and s["blk"] == blk and s["it"] == it), None)

    @property
    def n_blocks(self):
        return -(-self.n_sub // BLOCK)


# ---- content ---------------------------------------------------------------------------------------------------------------------
def skewed(seed, w, h, c, p=0.55, spread=256):
    """An image whose Up-filtered bytes are drawn from a geometric distribution over 0, 1, 255, 2, 254, ...: literals whose codes
    have every length a table allows (the 1-pass tables by design, a 2-pass table by the histogram), few matches."""
    rng = np.random.default_rng(seed)
    k = np.minimum(rng.geometric(1.0 - p, (h, w * c)) - 1, spread - 1)
    f = np.where(k & 1, (k + 1) // 2, 256 - k // 2).astype(np.uint8)  # 0, 1, 255, 2, 254, ...
    return np.cumsum(f, axis=0, dtype=np.uint64).astype(np.uint8).reshape(h, w, c)


def stripes(period, w, h, c, ramp=7):
    """test_decode_model.periodic_images cut down: vertical stripes on a vertical ramp -- every filtered row the same few bytes, a
    stream that keeps a decoder that began at a wrong bit in a stable false phase"""
    pal = np.random.default_rng(period).integers(0, 256, (period, c), dtype=np.uint8)
    return np.ascontiguousarray((pal[np.arange(w) % period][None] + (np.arange(h)[:, None, None] * ramp).astype(np.uint8)).astype(np.uint8))


def stacked(*parts):
    """images of one width and channel count, one under the other"""
    return np.ascontiguousarray(np.concatenate(parts, axis=0))


def content(recipe):
    """an image (h, w, c) from its recipe: a tuple that names the content and its parameters, ("stack", recipe, ...) for several"""
    import fpng_amd
    import ui_images
    kind, *a = recipe
    if kind == "stack":
        return stacked(*[content(r) for r in a])
    if kind == "skew":
        return skewed(*a)
    if kind == "stripes":
        return stripes(*a)
    if kind in ("glyphs", "panels", "dither"):
        seed, w, h, c = a
        return np.ascontiguousarray(getattr(ui_images, kind)(w, h, c, seed=seed))
    if kind == "photo":  # a crop of tests/real_image.py's photograph
        import dropin
        import real_image
        x, y, w, h = a
        rgb = real_image.rgb_pixels(dropin.decode)
        assert y + h <= rgb.shape[0] and x + w <= rgb.shape[1]
        return np.ascontiguousarray(rgb[y:y + h, x:x + w])
    seed, w, h, c = a  # "grad", "blocks", "solid"
    return np.asarray(fpng_amd.synth_image(kind, w, h, c, seed=seed))


def encode(img, flags):
    h, w, c = img.shape
    png = oracle().encode(np.ascontiguousarray(img).reshape(-1), w, h, c, flags)
    assert png is not None
    return png


def large(png):
    dm = _dm()
    return TM.LargeStream(png, dm.plan, dm.emul())


def retimed(png, delta, rows=None):
    """The file with its end-of-block code `delta` bits later (earlier: < 0): non-filter literals, from the stream's end backwards
    (of the last `rows` rows only), swapped for byte values whose codes differ in length.  None if the literals there cannot make
    up `delta`."""
    if delta == 0:
        return png
    s = large(png)
    by_len = {}
    for b, (_, l) in sorted(s.lit_code.items()):
        by_len.setdefault(l, b)
    lens = sorted(by_len)
    lo = 0 if rows is None else int(np.searchsorted(s.out_pos, (s.h - rows) * s.stride))
    new, left, i = [], delta, s.n - 1
    while left and i > lo:
        i -= 1
        t = s.token(i)
        if t[0] == "lit" and int(s.out_pos[i]) % s.stride:
            l0 = s.lit_code[t[1]][1]
            l1 = min(lens, key=lambda l: (abs(left - (l - l0)), l))
            if l1 != l0:
                t, left = ("lit", by_len[l1]), left - (l1 - l0)
        new.append(t)
    if left:
        return None
    return s.splice(i, s.n - 1, new[::-1])


def rewritten(png, first_row, n_rows, value_of):
    """token_mutator.Stream.write: rows [first_row, first_row + n_rows) of the file as literals alone -- the row's filter literal,
    then value_of(y, j) for every byte j of the row"""
    s = TM.Stream(png, _dm().plan)
    pos = s.positions()
    a = next(i for i, p in enumerate(pos) if p >= first_row * s.stride)
    b = next(i for i, p in enumerate(pos) if p >= (first_row + n_rows) * s.stride)
    assert pos[a] == first_row * s.stride and pos[b] == (first_row + n_rows) * s.stride  # (no match crosses a row's end)
    mid = []
    for y in range(first_row, first_row + n_rows):
        mid.append(("lit", 2 if y else 0))
        mid += [("lit", value_of(y, j)) for j in range(s.stride - 1)]
    return s.write(s.tokens[:a] + mid + s.tokens[b:]), s


# ---- the properties ---------------------------------------------------------------------------------------------------------------
def _border_end(tr, how, where):
    """the end-of-block code at a subsequence border: begins on it, ends on it, straddles it; `where`: a border inside a workgroup's
    block, or the one between block 0 and block 1"""
    E, L = tr.E, tr.L
    if how == "begins":
        ok, border = E % SUB == 0, E // SUB
    elif how == "ends":
        ok, border = (E + L) % SUB == 0, (E + L) // SUB
    else:
        ok, border = E % SUB > SUB - L, E // SUB + 1
    return tr.status == 0 and ok and border > 0 and (border == BLOCK if where == "block" else border % BLOCK != 0)


def _last_sub(tr, n_sub, form=None):
    """n_sub subsequences; form: the last one holds only the code's tail ("tail"), only the padding bits behind the code ("padding")"""
    if tr.status != 0 or tr.n_sub != n_sub:
        return False
    last = (n_sub - 1) * SUB
    return form is None or (tr.E < last < tr.E + tr.L if form == "tail" else tr.E + tr.L <= last)


def _steps0(tr):
    return [s for s in tr.steps if s["round"] == 0 and s["kind"] == KIND_REDO]


def _need0(tr, lo, hi):
    """a block whose step 0 of round 0 has lo <= n_need <= hi (0: no step at all)"""
    if tr.status != 0:
        return False
    if hi == 0:
        return any(b["round"] == 0 and not tr.need(b["blk"]) for b in tr.blocks)
    return any(s["it"] == 0 and lo <= s["n_need"] <= hi for s in _steps0(tr))


def _settled0(tr, blk):
    return tr.block(blk, 0)["left"] == 0


def _border_open(tr, many):
    """a block that round 0 settled and a border round opens: every step there with n_need < 4 / a step with n_need >= 4"""
    for b in tr.blocks:
        if b["round"] >= 1 and _settled0(tr, b["blk"]):
            need = [s["n_need"] for s in tr.steps if s["round"] == b["round"] and s["blk"] == b["blk"] and s["kind"] == KIND_REDO]
            if need and (max(need) >= GATHER_MIN if many else max(need) < GATHER_MIN):
                return tr.status == 0
    return False


def _gathered(tr):
    return [s for s in _steps0(tr) if s["n_need"] >= GATHER_MIN]


PROPS = {}
for _pass in ("1pass", "2pass"):
    for _how in ("begins", "ends", "straddles"):
        for _where in ("inner", "block"):
            PROPS[f"A.end.{_how}.{_where}.{_pass}"] = functools.partial(_border_end, how=_how, where=_where)
for _n in (1, 2, 511, 512, 1024):
    PROPS[f"A.n_sub.{_n}"] = functools.partial(_last_sub, n_sub=_n)
for _n in (513, 1025):
    for _form in ("tail", "padding"):
        PROPS[f"A.n_sub.{_n}.{_form}"] = functools.partial(_last_sub, n_sub=_n, form=_form)
PROPS.update({
    "A.first_bit.0": lambda tr: tr.status == 0 and tr.first_bit % 32 == 0,
    "A.first_bit.1": lambda tr: tr.status == 0 and tr.first_bit % 32 == 1,
    "A.first_bit.31": lambda tr: tr.status == 0 and tr.first_bit % 32 == 31,
    "A.first_bit.between": lambda tr: tr.status == 0 and 1 < tr.first_bit % 32 < 31,
    "B.need0.0": functools.partial(_need0, lo=0, hi=0),
    "B.need0.1": functools.partial(_need0, lo=1, hi=1),
    "B.need0.2": functools.partial(_need0, lo=2, hi=2),
    "B.need0.3": functools.partial(_need0, lo=3, hi=3),
    "B.need0.4": functools.partial(_need0, lo=4, hi=4),
    "B.need0.5_to_63": functools.partial(_need0, lo=5, hi=63),
    "B.need0.64": functools.partial(_need0, lo=64, hi=64),
    "B.need0.65": functools.partial(_need0, lo=65, hi=65),
    "B.need0.over_128": functools.partial(_need0, lo=129, hi=BLOCK),
    "B.steps.second": lambda tr: tr.status == 0 and any(b["round"] == 0 and b["left"] == 0 and len(tr.need(b["blk"])) == 2 for b in tr.blocks),
    "B.steps.third": lambda tr: tr.status == 0 and any(b["round"] == 0 and b["left"] == 0 and len(tr.need(b["blk"])) == 3 for b in tr.blocks),
    "B.left_crawling.settled_by_maps": lambda tr: tr.status == 0 and any(b["round"] == 0 and b["left"] == LEFT_CRAWLING and (tr.block(b["blk"], 1) or {}).get("maps") == 1
                                                                         for b in tr.blocks),
    # (the border rounds' kernel is another instance of the template: its gather runs only for blocks that round 0 left crawling)
    "B.left_crawling.gathered_in_round_1": lambda tr: tr.status == 0 and any(b["round"] == 0 and b["left"] == LEFT_CRAWLING and (tr.step(b["blk"], 0, 1) or {}).get("kind") == KIND_REDO
                                                                             and tr.step(b["blk"], 0, 1)["n_need"] >= GATHER_MIN for b in tr.blocks),
    "B.border.open.under_4": functools.partial(_border_open, many=False),
    "B.border.open.4_and_more": functools.partial(_border_open, many=True),
    "B.gather.every_wave": lambda tr: tr.status == 0 and any({t // WAVE for t in s["threads"]} == set(range(BLOCK // WAVE)) for s in _gathered(tr)),
    "B.gather.short_last_block": lambda tr: tr.status == 0 and any(s["valid"] < WAVE and s["blk"] == tr.n_blocks - 1 for s in _gathered(tr)),
    "B.gather.pass_ends_mid_wave": lambda tr: tr.status == 0 and any(s["n_need"] > WAVE and s["threads"][WAVE - 1] // WAVE == s["threads"][WAVE] // WAVE
                                                                     and s["threads"][WAVE] % WAVE < WAVE - 1 for s in _gathered(tr)),
    "D.walks.4": lambda tr: tr.status == 0 and tr.c == 4 and tr.max_walks == max_walks(4) <= MAX_WALKS_PER_ROW,
    "D.walks.3": lambda tr: tr.status == 0 and tr.c == 3 and tr.max_walks == max_walks(3) <= MAX_WALKS_PER_ROW,
    "D.min_bytes": lambda tr: tr.status == 0 and tr.min_bytes == MIN_SUB_BYTES,
})
# group C's properties are a batch's (`Batch.holds`): so many compressed files, stored files at those places
C_PROPS = ["C.batch.1", "C.batch.63", "C.batch.64", "C.batch.65", "C.batch.64.no_stored", "C.batch.65.no_stored", "C.files.64.with_stored", "C.stored.first",
           "C.stored.middle", "C.stored.last"]
ALL_PROPS = sorted(PROPS) + C_PROPS
UNREACHABLE = {
    # In a border round the threads of a block that round 0 SETTLED start where their predecessors end, all but thread 0, which takes
    # the start the border asks for: step 0 has one thread to correct.  Decoding thread t again changes only thread t's end, so
    # step k + 1 has at most thread t + 1 to correct: n_need is 1 in every step, until, after kRefixRounds of them, the phase maps
    # are used -- and those set every thread right whose predecessors' maps know its phase.  kGatherMin and more in a border round
    # are had only by a block that round 0 left kLeftCrawling (B.left_crawling.settled_by_maps: its step 0 there is gathered).
    # A search over 40 000 periodic and noisy-periodic images (1- and 2-pass, two to six blocks each) found no settled block with
    # more than one; the few that reached their phase maps there (last blocks of four or five threads) had none left behind them.
    "B.border.open.4_and_more": "a settled block's corrections in a border round go one thread per step",
}


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
class Case:
    """one file: name, group, the properties it was built for, and how it is built (`make` -> the file's bytes)"""

    def __init__(self, name, props, make):
        self.name, self.group, self.props, self.make = name, name[0], list(props), make
        self._png = self._trace = None

    @property
    def png(self):
        if self._png is None:
            self._png = self.make()
            assert self._png is not None, self.name
        return self._png

    @property
    def trace(self):
        if self._trace is None:
            self._trace = Trace(self.png)
        return self._trace

    def missing(self):
        """the properties of its name that the trace does not show"""
        return [p for p in self.props if not PROPS[p](self.trace)]

    def __repr__(self):
        return self.name


def _ended(recipe, flags, target, rows=None):
    """the recipe's file with its end-of-block code moved to target(L, E): bits behind first_bit, from the code's length and where
    it begins in the file as the encoder wrote it"""
    def make():
        png = encode(content(recipe), flags)
        tr = Trace(png)
        return retimed(png, target(tr.L, tr.E) - tr.E, rows)
    return make


def _plain(recipe, flags):
    return lambda: encode(content(recipe), flags)


# What the searches found (tools of a session, not kept: recipes drawn from seeds until the trace showed the property).  Sizes of the
# "skew" recipes: the height at which the code's first bit comes nearest to the border aimed at; `retimed` does the rest.
_SKEW_AT = {  # (flags, border in subsequences) -> recipe
    (0, 512): ("skew", 7, 160, 117, 4, 0.6), (1, 512): ("skew", 7, 160, 162, 4, 0.6),
    (0, 1024): ("skew", 7, 160, 234, 4, 0.6), (1, 1024): ("skew", 7, 160, 324, 4, 0.6),
    (0, 511): ("skew", 7, 160, 163, 3, 0.6), (1, 511): ("skew", 7, 160, 213, 3, 0.6),
}
_INNER = {0: ("skew", 1, 100, 60, 3, 0.55), 1: ("skew", 2, 100, 60, 4, 0.7)}


def group_a():
    out = []
    for flags, pname in ((0, "1pass"), (1, "2pass")):
        for how, at in (("begins", lambda L: 0), ("ends", lambda L: -L), ("straddles", lambda L: -(L // 2))):
            # (the inner border aimed at: the nearest in front of the file's end)
            out.append(Case(f"A.end.{how}.inner.{pname}", [f"A.end.{how}.inner.{pname}"], _ended(_INNER[flags], flags, lambda L, E, at=at: E // SUB * SUB + at(L))))
            props = [f"A.end.{how}.block.{pname}"]
            # (the 1-pass tables' first_bit is 490 with four channels: no byte border, so a code that ends on the border has padding behind it)
            props += ["A.n_sub.513.tail"] if how == "straddles" else (["A.n_sub.513.padding"] if how == "ends" and flags == 0 else [])
            out.append(Case(f"A.end.{how}.block.{pname}", props, _ended(_SKEW_AT[flags, 512], flags, lambda L, E, at=at: BLOCK * SUB + at(L))))
    mid = lambda n: (lambda L, E: (n - 1) * SUB + SUB // 2 - L)  # n subsequences, the code in the middle of the last one
    out.append(Case("A.n_sub.1", ["A.n_sub.1", "A.first_bit.0"], _plain(("skew", 30, 8, 8, 3, 0.6), 1)))
    out.append(Case("A.n_sub.2", ["A.n_sub.2", "A.first_bit.1"], _plain(("skew", 37, 10, 8, 3, 0.6), 1)))
    out.append(Case("A.first_bit.31", ["A.first_bit.31"], _plain(("skew", 2, 40, 24, 4, 0.6), 1)))
    out.append(Case("A.n_sub.511", ["A.n_sub.511", "A.first_bit.between"], _ended(_SKEW_AT[0, 511], 0, mid(511))))
    out.append(Case("A.n_sub.512", ["A.n_sub.512"], _ended(_SKEW_AT[1, 512], 1, mid(512))))
    out.append(Case("A.n_sub.1024", ["A.n_sub.1024"], _ended(_SKEW_AT[0, 1024], 0, mid(1024))))
    out.append(Case("A.n_sub.1025.tail", ["A.n_sub.1025.tail"], _ended(_SKEW_AT[1, 1024], 1, lambda L, E: 2 * BLOCK * SUB - L // 2)))
    out.append(Case("A.n_sub.1025.padding", ["A.n_sub.1025.padding"], _ended(_SKEW_AT[0, 1024], 0, lambda L, E: 2 * BLOCK * SUB - L)))
    return out


_B_FOUND = [  # (properties, recipe, flags)
    (["B.need0.0"], ("panels", 1, 675, 68, 3), 1),
    (["B.need0.1", "B.need0.2"], ("stack", ("skew", 3, 463, 66, 4, 0.6), ("stripes", 10, 463, 176, 4)), 0),
    (["B.need0.3"], ("stack", ("skew", 20, 1105, 18, 4, 0.6), ("stripes", 18, 1105, 64, 4)), 0),
    (["B.need0.4"], ("stripes", 10, 1305, 57, 4), 0),
    (["B.need0.5_to_63"], ("glyphs", 2, 479, 159, 4), 0),
    (["B.need0.64"], ("glyphs", 356, 538, 207, 3), 0),
    (["B.need0.65"], ("glyphs", 475, 735, 194, 3), 0),
    (["B.need0.over_128"], ("stripes", 2, 4096, 300, 4), 1),
    (["B.steps.second"], ("glyphs", 34, 823, 87, 3), 0),
    (["B.steps.third"], ("glyphs", 81, 426, 215, 3), 0),
    (["B.left_crawling.settled_by_maps", "B.left_crawling.gathered_in_round_1"], ("stripes", 14, 2303, 135, 3), 1),
    (["B.border.open.under_4"], ("glyphs", 540, 556, 187, 3), 0),
    (["B.gather.every_wave"], ("glyphs", 168, 323, 185, 3), 0),
    (["B.gather.short_last_block"], ("stripes", 26, 1071, 57, 3), 1),
    (["B.gather.pass_ends_mid_wave"], ("stripes", 22, 1085, 159, 4), 1),
]


def group_b():
    return [Case(props[0], props, _plain(recipe, flags)) for props, recipe, flags in _B_FOUND]


def _twelve_bit_rows(seed, c, first_row=20, n_rows=4):
    """Group D: a 2-pass file of a skewed image 256 pixels wide (its rare byte values get the longest codes a table may have), rows
    [first_row, first_row + n_rows) rewritten as literals of 12 bits alone: 256 * c * 12 bits are whole subsequences (24 or 18), so
    every such row puts out the fewest bytes a subsequence can.  A window reaches max_walks(c) when its row's filter literal is the
    LAST token of its subsequence: literals in front of the rows are swapped until the second row's filter literal begins in a
    subsequence's last bit."""
    def make():
        base = encode(skewed(seed, 256, 40, c, 0.6), 1)
        probe = TM.Stream(base, _dm().plan)
        longest = sorted(b for b, (_, l) in probe.lit_code.items() if l == MAX_CODE_BITS)
        assert longest, "the table has no literal of 12 bits"
        png, s = rewritten(base, first_row, n_rows, lambda y, j: longest[(y + j) % len(longest)])
        ls = large(png)
        i = int(np.searchsorted(ls.out_pos, (first_row + 1) * ls.stride))
        assert ls.token(i) == ("lit", 2)
        rel = (int(ls.bitpos[i]) - ls.first) % SUB
        # (later by (SUB - 1 - rel) bits; `retimed` works from the end, so: the rows in front, as a file of their own tokens)
        by_len = {}
        for b, (_, l) in sorted(s.lit_code.items()):
            by_len.setdefault(l, b)
        lens, left = sorted(by_len), (SUB - 1 - rel) % SUB
        T = list(TM.Stream(png, _dm().plan).tokens)
        pos = s.positions(T)
        k = next(q for q, p in enumerate(pos) if p >= first_row * s.stride)
        while left and k > 0:
            k -= 1
            if T[k][0] == "lit" and pos[k] % s.stride:
                l0 = s.lit_code[T[k][1]][1]
                l1 = min(lens, key=lambda l: (abs(left - (l - l0)), l))
                T[k], left = ("lit", by_len[l1]), left - (l1 - l0)
        assert not left
        return s.write(T)
    return make


def group_d():
    return [Case("D.walks.4", ["D.walks.4", "D.min_bytes"], _twelve_bit_rows(11, 4)), Case("D.walks.3", ["D.walks.3", "D.min_bytes"], _twelve_bit_rows(12, 3))]


class Batch:
    """Group C: `n` compressed files -- most with 1 to 3 subsequences, `two_blocks` of them group A's files of 513 subsequences --
    and stored files (no subsequences: they share their successor's sub_base) at the places `stored`: "first", "middle", "last"."""

    def __init__(self, name, n, stored, two_blocks):
        self.name, self.group, self.n, self.stored = name, "C", n, list(stored)
        self.props = [name] + [f"C.stored.{s}" for s in stored]
        small = []
        for k in range(n - len(two_blocks)):
            w, h = ((7, 7), (8, 8), (10, 8), (12, 10))[k % 4]  # (smaller ones come out as stored files)
            small.append(encode(skewed(1000 + k, w, h, 3 + k % 2, 0.6), k % 2))
        files = list(small)
        for j, case in enumerate(two_blocks):  # spread over the batch
            files.insert((j + 1) * len(files) // (len(two_blocks) + 1), case.png)
        raw = lambda k: encode(skewed(2000 + k, 9, 7, 3 + k % 2, 0.6), 2)
        if "first" in stored:
            files.insert(0, raw(0))
        if "middle" in stored:
            files.insert(len(files) // 2, raw(1))
            files.insert(len(files) // 2, raw(2))  # (two in a row)
        if "last" in stored:
            files.append(raw(3))
        self.files = files
        self.modes = [_dm().plan(f)[1] for f in files]

    def holds(self):
        """-> the properties of its name that the files do not have"""
        comp = [f for f, m in zip(self.files, self.modes) if not m]
        n_sub = [Trace(f).n_sub for f in comp]
        ok = len(comp) == self.n and sum(1 <= v <= 3 for v in n_sub) >= self.n - 3 and (self.n < 63 or sum(v > BLOCK for v in n_sub) >= 2)
        ok = ok and (not self.name.startswith("C.files.64") or len(self.files) == 64)
        at = [i for i, m in enumerate(self.modes) if m]
        want = {"first": [0], "middle": [i for i in at if 0 < i < len(self.files) - 1], "last": [len(self.files) - 1]}
        ok_stored = all(want[s] and set(want[s]) <= set(at) for s in self.stored) and (bool(at) == bool(self.stored))
        return [] if ok and ok_stored else list(self.props)

    def __repr__(self):
        return self.name


def group_c(a_cases):
    two = [c for c in a_cases if c.name in ("A.end.straddles.block.1pass", "A.end.ends.block.2pass")]
    every = ["first", "middle", "last"]
    return [Batch("C.batch.1", 1, [], []), Batch("C.batch.63", 63, every, two), Batch("C.batch.64", 64, every, two), Batch("C.batch.65", 65, every, two),
            Batch("C.batch.64.no_stored", 64, [], two), Batch("C.batch.65.no_stored", 65, [], two),
            # (63 to 65 compressed files and four stored ones are more than 64 files, the binary search's; here the ballot meets stored files)
            Batch("C.files.64.with_stored", 60, every, two)]


@functools.lru_cache(maxsize=None)
def all_cases():
    """-> {"A": [Case], "B": [Case], "C": [Batch], "D": [Case]}, built once"""
    a = group_a()
    return {"A": a, "B": group_b(), "C": group_c(a), "D": group_d()}
