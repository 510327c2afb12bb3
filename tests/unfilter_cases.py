"""The un-filter pass's and the pixel expansion's designed files (test_png_unfilter_cpu.py, test_gpu_decode_png_unfilter.py,
test_gpu_decode_png_host.py), written row by row with filter_writer.py: predictor classes, dependency chains, shapes at the band's
and the tile's edges, the kernel's own two refusals by position, the expansion table.  Every list is made once; streams are zlib's
at level 1; no file's scanlines exceed 1 MiB.  What a file is expected to give is the plain model's answer (Case.expected), which
the CPU test ties to Pillow."""
import functools
import struct
import zlib

import numpy as np

import filter_writer as fw
import png_cases as pc

COLOR_OF_BPP = {1: 0, 2: 4, 3: 2, 4: 6}
MAX_SCAN = 1 << 20


class Case:
    """name, file, status (0, or the refusal's); w, h, color; scan (the scanlines), recon (the model's reconstructed bytes; None for
    a refusal), pixels (what the writer was given, None where it was given filtered bytes), plte / trns (the chunks that count,
    or None), log (filter_writer.Log), reaches (c: what the file is listed for), neighbour (d: the accepted file's name)"""

    def __init__(self, name, w, h, color, scan, recon, log, pixels=None, plte=None, trns=None, status=0, reaches=None, neighbour=None, chunks=None):
        """chunks: png_cases.png's arguments for the file's PLTE / tRNS chunks where they are not simply plte and trns"""
        assert len(scan) == h * (1 + w * fw.BPP[color]) <= MAX_SCAN, name
        self.name, self.w, self.h, self.color, self.scan, self.recon, self.log, self.pixels = name, w, h, color, scan, recon, log, pixels
        self.plte, self.trns, self.status, self.reaches, self.neighbour = plte, trns, status, reaches or {}, neighbour
        self.file = pc.png(w, h, color, zlib.compress(scan, 1), **(dict(plte=plte, trns=trns) if chunks is None else chunks))
        self._expected = {}

    @property
    def dims(self):
        return self.w, self.h

    @property
    def channels(self):
        return fw.channels_in_file(self.color, self.trns)

    def expected(self, desired):
        """the model's pixels, (h, w, desired) uint8"""
        if desired not in self._expected:
            self._expected[desired] = fw.expand(self.recon, self.color, self.plte, self.trns, desired)
        return self._expected[desired]

    def __iter__(self):  # (name, file) or (name, file, status)
        return iter((self.name, self.file, self.status) if self.status else (self.name, self.file))


def _mix(rng, h, n):
    """some structure and some noise, so that every filter has work"""
    y, x = np.mgrid[0:h, 0:n]
    smooth = ((x * 5 + y * 3) & 255).astype(np.uint8)
    return np.where(rng.integers(0, 3, (h, n)) == 0, rng.integers(0, 256, (h, n), dtype=np.uint8), smooth).astype(np.uint8)


def _palette(seed, entries=256):
    return np.random.default_rng(seed).integers(0, 256, 3 * entries, dtype=np.uint8).tobytes()


def _from_pixels(name, w, h, color, pixels, filters, **kw):
    scan, recon, log = fw.from_pixels(pixels, fw.BPP[color], filters)
    return Case(name, w, h, color, scan, recon, log, pixels=pixels, **kw)


# ---- a. predictor classes ----
ALPHABET = (0, 1, 2, 3, 127, 128, 129, 253, 254, 255)
PREDICTOR_SEEDS = {1: 25, 2: 87, 3: 52, 4: 0}  # first_covering_seed(bpp), which the CPU test holds against this


def predictor_filters(h=66):
    """Paeth in rows 0 and 64, Average in 63, every type somewhere"""
    f = [(4, 1, 2, 3)[y % 4] for y in range(h)]
    f[62] = 0
    return f


def predictor_case(bpp, seed):
    w, h = 70, 66
    rng = np.random.default_rng(1000 * bpp + seed)
    n = w * bpp
    px = np.array(ALPHABET, np.uint8)[rng.integers(0, len(ALPHABET), (h, n))]
    px = np.where(rng.integers(0, 5, (h, n)) == 0, rng.integers(0, 256, (h, n), dtype=np.uint8), px).astype(np.uint8)
    return _from_pixels(f"predictors_bpp{bpp}", w, h, COLOR_OF_BPP[bpp], px, predictor_filters(h))


def covers_predictors(log, bpp, reachable):
    """every reachable Paeth class, in general and in row 64; every Average class; Sub and Up with and without a wrap"""
    return (log.pred[(4, bpp)] == reachable and log.band_top_paeth[bpp] == reachable and log.pred[(3, bpp)] == fw.AVERAGE_CLASSES
            and log.pred[(1, bpp)] == fw.WRAP_CLASSES and log.pred[(2, bpp)] == fw.WRAP_CLASSES)


def first_covering_seed(bpp, reachable, seeds=range(128)):
    return next(s for s in seeds if covers_predictors(predictor_case(bpp, s).log, bpp, reachable))


@functools.lru_cache(None)
def predictor_cases():
    return [predictor_case(bpp, PREDICTOR_SEEDS[bpp]) for bpp in (1, 2, 3, 4)]


# ---- b. dependency chains: files given as filtered bytes ----
@functools.lru_cache(None)
def chain_cases():
    out = []
    w, h = 200, 70
    for filt in (1, 2, 3, 4):
        for bpp in (1, 2, 3, 4):
            const = (0x01, 0x80, 0xFF)[(filt + bpp) % 3]
            scan, recon, log = fw.from_filtered(np.full((h, w * bpp), const, np.uint8), bpp, [filt] * h)
            out.append(Case(f"chain_f{filt}_bpp{bpp}_{const:02x}", w, h, COLOR_OF_BPP[bpp], scan, recon, log))
    for bpp in (1, 2, 3, 4):
        rng = np.random.default_rng(2000 + bpp)
        scan, recon, log = fw.from_filtered(rng.integers(0, 256, (h, w * bpp), dtype=np.uint8), bpp, rng.integers(0, 5, h).tolist())
        out.append(Case(f"chain_random_bpp{bpp}", w, h, COLOR_OF_BPP[bpp], scan, recon, log))
    return out


# ---- c. shapes outside the grid of png_cases.shape_cases ----
def _shape(k, w, h, color, reaches):
    rng = np.random.default_rng(3000 + k)
    plte = _palette(3100 + k) if color == 3 else None
    return _from_pixels(f"shape_{w}x{h}_c{color}", w, h, color, _mix(rng, h, w * fw.BPP[color]), rng.integers(0, 5, h).tolist(), plte=plte, reaches=reaches)


@functools.lru_cache(None)
def shape_cases():
    """reaches: what the CPU test asserts from the file's log -- positions (a set that must be met), bands, tiles, last_steps (a
    value that must be among the bands' last steps mod 64), row_bytes_above"""
    out, rnd = [], (0, 4, 2, 6, 3)
    both = {"band_top", "band_bottom", "partial_last"}
    for h in (64, 65):  # the second tile edge and the skew across it: a full band's last step is w + 62
        for w in (127, 128, 129, 130):
            out.append(_shape(len(out), w, h, rnd[len(out) % 5], dict(bands=h - 63, tiles=(w + 62) // 64 + 1, last_steps=(w + 62) % 64,
                                                                     positions=both if h == 65 else {"tile_first", "tile_last", "x%64=63"})))
    for h in (127, 128, 191, 192, 193):  # the third band's edge
        out.append(_shape(len(out), 70, h, rnd[len(out) % 5], dict(bands=(h + 63) // 64, tiles=3, positions={"band_top", "band_bottom"} | ({"partial_last"} if h % 64 else set()))))
    out.append(_shape(len(out), 4097, 3, 6, dict(bands=1, tiles=65, positions={"partial_last", "tile_first", "tile_last"})))
    out.append(_shape(len(out), 40000, 1, 0, dict(bands=1, tiles=625, row_bytes_above=32768)))  # a row longer than the inflate window
    out.append(_shape(len(out), 8200, 2, 6, dict(bands=1, tiles=129, row_bytes_above=32768)))   # rows of 32801 bytes with their filter byte
    out.append(_shape(len(out), 1, 4097, 0, dict(bands=65, tiles=1, last_steps=63, positions={"band_top", "band_bottom", "partial_last"})))
    out.append(_shape(len(out), 2, 4097, 4, dict(bands=65, tiles=2, last_steps=0, positions={"band_top", "band_bottom", "partial_last"})))
    out.append(_shape(len(out), 3, 1000, 2, dict(bands=16, tiles=2, last_steps=1, positions={"band_top", "band_bottom", "partial_last"})))
    out.append(_shape(len(out), 1000, 128, 2, dict(bands=2, tiles=17, positions={"band_top", "band_bottom"}, not_positions={"partial_last"})))
    out.append(_shape(len(out), 1000, 129, 2, dict(bands=3, tiles=17, positions={"band_top", "band_bottom", "partial_last"})))
    return out


# ---- d. the un-filter kernel's own refusals, by position: all INVALID_IDAT ----
def _bad_scan(case, at, value, name):
    scan = bytearray(case.scan)
    assert scan[at] != value
    scan[at] = value
    return Case(name, case.w, case.h, case.color, bytes(scan), None, None, plte=case.plte, status=pc.INVALID_IDAT, neighbour=case.name)


@functools.lru_cache(None)
def _refusals():
    good, bad = [], []
    w = 70
    for k, h in enumerate((1, 64, 65, 130)):  # a filter byte of 5 and of 255: lane 0, lane 63, band 1, the last row
        color = (0, 4, 2, 6)[k]
        rng = np.random.default_rng(4000 + h)
        g = _from_pixels(f"filters_ok_h{h}", w, h, color, _mix(rng, h, w * fw.BPP[color]), rng.integers(0, 5, h).tolist())
        good.append(g)
        for y in sorted({y for y in (0, 63, 64, h - 1) if y < h}):
            for value in (5, 255):
                bad.append(_bad_scan(g, y * (1 + w * fw.BPP[color]), value, f"filter_{value}_h{h}_row{y}"))
    # a palette index equal to PLTE's entry count.  The rows of the five places have Up (and the row below each has Sub; row 64,
    # which is both, has None), so that the one pixel changes one byte of the scanlines
    h = 130
    places = (("first", 0, 0), ("row63", 63, 37), ("row64", 64, 5), ("row129", 129, 33), ("last", 129, w - 1))
    for entries in (10, 1, 2, 255, 256):
        rng = np.random.default_rng(4100 + entries)
        filters = rng.integers(0, 5, h).tolist()
        filters[0], filters[1], filters[63], filters[64], filters[65], filters[129] = 2, 1, 2, 0, 1, 2
        px = rng.integers(0, entries, (h, w)).astype(np.uint8)
        for _, y, x in places:
            px[y, x] = entries - 1  # (the highest index that is good: with 256 entries, 255)
        g = _from_pixels(f"palette{entries}_ok", w, h, 3, px, filters, plte=_palette(4200 + entries, entries))
        good.append(g)
        for place, y, x in places if entries < 256 else ():
            bad.append(_bad_scan(g, y * (1 + w) + 1 + x, (g.scan[y * (1 + w) + 1 + x] + 1) & 255, f"palette{entries}_index_{place}"))
    return good, bad


def refusal_cases():
    """(name, file, INVALID_IDAT) each; .neighbour names the accepted file that differs in one byte of the scanlines"""
    return _refusals()[1]


def neighbour_cases():
    return _refusals()[0]


# ---- e. the expansion table ----
RGB_KEYS = [(0, 0, 0, 0), (255, 255, 255, 0), (10, 200, 30, 0), (10, 200, 30, 0x01), (10, 200, 30, 0x7F), (10, 200, 30, 0xFF)]  # r, g, b, high byte
GREY_KEYS = (0, 1, 127, 255, 0x1280)


def _rgb_key_image(key, seed, w=24, h=80):
    """the key, every permutation of its bytes, and for each pair of channels a pixel that equals the key in exactly those two:
    each of the nine at x = 0 and at x = w - 1, in rows 2 .. 10 and, in the second band, 66 .. 74"""
    rng = np.random.default_rng(seed)
    px = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    r, g, b = key
    special = [(r, g, b), (r, b, g), (g, r, b), (g, b, r), (b, r, g), (b, g, r), (r, g, b ^ 0x80), (r, g ^ 1, b), (r ^ 0xFF, g, b)]
    for base in (2, 66):
        for k in range(9):
            px[base + k, 0], px[base + k, w - 1] = special[k], special[(k + 4) % 9]
    return px.reshape(h, w * 3)


@functools.lru_cache(None)
def expansion_cases():
    out = []
    rng = np.random.default_rng(5000)
    w, h = 24, 70

    def add(name, color, pixels, **kw):
        out.append(_from_pixels(name, w, len(pixels), color, pixels, rng.integers(0, 5, len(pixels)).tolist(), **kw))

    for key in GREY_KEYS:
        px = rng.integers(0, 256, (h, w), dtype=np.uint8)
        px[0, 0] = px[h - 1, w - 1] = key & 255
        px.reshape(-1)[1 + rng.permutation(w * h - 2)[:256]] = np.arange(256, dtype=np.uint8)  # every value occurs
        add(f"grey_key_{key:04x}", 0, px, trns=struct.pack(">H", key))
    for k, (r, g, b, hi) in enumerate(RGB_KEYS):
        add(f"rgb_key_{r}_{g}_{b}_hi{hi:02x}", 2, _rgb_key_image((r, g, b), 5100 + k, w), trns=struct.pack(">HHH", hi << 8 | r, hi << 8 | g, hi << 8 | b))
    px = rng.integers(0, 256, (h, w, 2), dtype=np.uint8)
    for k, ga in enumerate((g, a) for g in (0, 255) for a in (0, 1, 254, 255)):
        px[k, 0], px[65, k], px[k + 8, w - 1] = ga, ga, ga
    add("grey_alpha_edges", 4, px.reshape(h, -1))
    idx = rng.integers(0, 256, (h, w), dtype=np.uint8)
    idx[0, :4], idx[h - 1, -4:] = (0, 1, 254, 255), (0, 1, 254, 255)
    for n in (0, 1, 255, 256):
        add(f"palette256_trns{n}", 3, idx, plte=_palette(5200), trns=bytes((7 + 37 * i) & 255 for i in range(n)))
    idx10 = rng.integers(0, 10, (h, w)).astype(np.uint8)
    plte10, trns20 = _palette(5201, 10), bytes((200 - 9 * i) & 255 for i in range(20))
    add("palette10_trns20", 3, idx10, plte=plte10, trns=trns20)
    # chunk order, and chunks where they have no meaning
    add("trns_in_front_of_plte", 3, idx10, plte=plte10, trns=trns20[:10], chunks=dict(before_plte=[pc.chunk(b"tRNS", trns20[:10])], plte=plte10))
    add("two_plte_chunks", 3, idx10, plte=plte10, chunks=dict(before_plte=[pc.chunk(b"PLTE", _palette(5202, 200))], plte=plte10))  # the last one counts
    rgb, rgba = rng.integers(0, 256, (h, w * 3), dtype=np.uint8), rng.integers(0, 256, (h, w * 4), dtype=np.uint8)
    add("plte_in_rgb", 2, rgb, chunks=dict(plte=_palette(5203, 16)))
    add("plte_in_rgb_not_multiple_of_3", 2, rgb, chunks=dict(plte=_palette(5203, 16)[:47]))
    add("plte_in_rgba", 6, rgba, chunks=dict(plte=_palette(5204, 256)))
    ga = rng.integers(0, 256, (h, w * 2), dtype=np.uint8)
    add("trns_in_grey_alpha", 4, ga, chunks=dict(trns=struct.pack(">H", int(ga[0, 0]))))  # ignored
    add("trns_in_rgba", 6, rgba, chunks=dict(trns=struct.pack(">HHH", *(int(v) for v in rgba[0, :3]))))
    return out


@functools.lru_cache(None)
def parity_cases():
    """the three files Pillow refuses and the tier takes (include/fpng_amd.h): a palette tRNS of 257 bytes is read up to 256, a grey
    tRNS of 1 byte and an RGB tRNS of 4 bytes are ignored.  Expected: the model's pixels, which the host twin must give as well."""
    rng = np.random.default_rng(6000)
    w, h = 24, 70
    idx = rng.integers(0, 256, (h, w), dtype=np.uint8)
    idx[0, 0], idx[h - 1, w - 1] = 255, 255
    grey, rgb = rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h, w * 3), dtype=np.uint8)
    return [_from_pixels("palette256_trns257", w, h, 3, idx, rng.integers(0, 5, h).tolist(), plte=_palette(6001), trns=bytes((11 + 29 * i) & 255 for i in range(257))),
            _from_pixels("grey_trns_1_byte", w, h, 0, grey, rng.integers(0, 5, h).tolist(), trns=bytes([int(grey[0, 0])])),
            _from_pixels("rgb_trns_4_bytes", w, h, 2, rgb, rng.integers(0, 5, h).tolist(), trns=bytes([0, int(rgb[0, 0]), 0, int(rgb[0, 1])]))]


def accepted_cases():
    """a - c and e: what the GPU tests decode in one batch"""
    return predictor_cases() + chain_cases() + shape_cases() + expansion_cases()
