"""A PNG scanline writer driven by rows, for the general decode tier's un-filter tests (unfilter_cases.py): the counterpart of
deflate_writer.py one layer up.  The caller gives the reconstructed pixels and a filter type per row, or the FILTERED bytes and a
filter type per row, and gets the scanlines, the reconstructed image and a log of what the predictors and the kernel's band
geometry meet on the way.  Nothing here reads a decoder, and nothing is shared with png_cases.filter_rows: the un-filter is the PNG
specification's (section 9, "Filtering"), serial, row by row and byte by byte in Python ints; the log is computed from its result,
so a test can assert what a file covers without asking the code under test.

    scan, recon, log = from_pixels(pixels, bpp, filters)      pixels: (h, w * bpp) uint8
    scan, recon, log = from_filtered(filtered, bpp, filters)  filtered: (h, w * bpp) uint8, the bytes behind each row's filter byte
    rgba = expand(recon, color, plte, trns, desired)          what the tier makes of the reconstructed bytes (include/fpng_amd.h)

The log (class Log):
    pred[(filter type, bytes per pixel)]   the set of predictor classes met:
        Sub (1), Up (2)    (wrapped,)                          raw + predictor went past 255
        Average (3)        (a + b >= 256, a + b odd, wrapped)
        Paeth (4)          (chosen 'a' | 'b' | 'c', pa == pb, pa == pc, pb == pc)
    band_top_paeth[bpp]   the Paeth classes met in rows y = 64, 128, ...: there b and c reach the kernel through memory (the row the
                          band above wrote back), not through the wave shuffle
    positions             the position classes the file's pixels fall into (POSITIONS below); t = x + (y mod 64) is the step at
                          which the kernel's skewed band works on pixel x of row y, 64 steps make a tile
    bands, tiles          bands of 64 rows; the largest number of tiles a band has
    last_steps            per band, (its last step) mod 64
    row_bytes             w * bpp"""
import numpy as np

BAND = 64  # rows of a band, steps of a tile (png_inflate_core.h: kBandRows, kTileSteps)
POSITIONS = ("x=0", "y=0", "band_top", "band_bottom", "partial_last", "x%64=0", "x%64=63", "tile_first", "tile_last")


class Log:
    def __init__(self):
        self.pred, self.band_top_paeth, self.positions = {}, {}, set()
        self.bands = self.tiles = self.row_bytes = 0
        self.last_steps = set()


def paeth(a, b, c):
    """the PaethPredictor of the specification, on Python ints"""
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    if pa <= pb and pa <= pc:
        return a
    if pb <= pc:
        return b
    return c


def unfilter(scan, w, h, bpp):
    """scanlines (a filter byte in front of each row) -> (h, w * bpp) uint8, or ValueError for a filter byte above 4"""
    n = w * bpp
    assert len(scan) == h * (n + 1)
    out = np.zeros((h, n), np.uint8)
    prev = bytes(n)
    for y in range(h):
        t = scan[y * (n + 1)]
        line = scan[y * (n + 1) + 1:(y + 1) * (n + 1)]
        cur = bytearray(n)
        if t == 0:
            cur[:] = line
        elif t == 1:
            for i in range(n):
                cur[i] = (line[i] + (cur[i - bpp] if i >= bpp else 0)) & 255
        elif t == 2:
            for i in range(n):
                cur[i] = (line[i] + prev[i]) & 255
        elif t == 3:
            for i in range(n):
                cur[i] = (line[i] + (((cur[i - bpp] if i >= bpp else 0) + prev[i]) >> 1)) & 255
        elif t == 4:
            for i in range(n):
                if i >= bpp:
                    cur[i] = (line[i] + paeth(cur[i - bpp], prev[i], prev[i - bpp])) & 255
                else:
                    cur[i] = (line[i] + paeth(0, prev[i], 0)) & 255
        else:
            raise ValueError(f"filter byte {t} in row {y}")
        out[y] = np.frombuffer(bytes(cur), np.uint8)
        prev = bytes(cur)
    return out


def _neighbours(recon, bpp):
    """a (left), b (above), c (above left) of every byte, int64, zeros outside the image"""
    r = recon.astype(np.int64)
    a, b, c = np.zeros_like(r), np.zeros_like(r), np.zeros_like(r)
    a[:, bpp:] = r[:, :-bpp]
    b[1:] = r[:-1]
    c[1:, bpp:] = r[:-1, :-bpp]
    return r, a, b, c


def _paeth_parts(a, b, c):
    """int64 arrays -> (chosen 0 | 1 | 2 for a | b | c, pa == pb, pa == pc, pb == pc)"""
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    chosen = np.where((pa <= pb) & (pa <= pc), 0, np.where(pb <= pc, 1, 2))
    return chosen, pa == pb, pa == pc, pb == pc


def _paeth_classes(parts):
    chosen, e_ab, e_ac, e_bc = parts
    codes = np.unique(chosen * 8 + e_ab * 4 + e_ac * 2 + e_bc)
    return {("abc"[k >> 3], bool(k & 4), bool(k & 2), bool(k & 1)) for k in codes.tolist()}


def reachable_paeth_classes():
    """every (a, b, c) of 0 .. 255: the Paeth classes that exist at all"""
    b, c = np.meshgrid(np.arange(256, dtype=np.int64), np.arange(256, dtype=np.int64), indexing="ij")
    out = set()
    for a in range(256):
        out |= _paeth_classes(_paeth_parts(np.int64(a), b, c))
    return out


AVERAGE_CLASSES = {(hi, odd, wrapped) for hi in (False, True) for odd in (False, True) for wrapped in (False, True)}
WRAP_CLASSES = {(False,), (True,)}


def filtered_of(recon, bpp, filters):
    """the forward filters of the specification: (h, n) uint8 of filtered bytes"""
    r, a, b, c = _neighbours(recon, bpp)
    t = np.asarray(filters, np.int64)[:, None]
    assert t.shape[0] == r.shape[0] and ((0 <= t) & (t <= 4)).all()
    chosen = _paeth_parts(a, b, c)[0]
    pae = np.where(chosen == 0, a, np.where(chosen == 1, b, c))
    pred = np.where(t == 0, 0, np.where(t == 1, a, np.where(t == 2, b, np.where(t == 3, (a + b) // 2, pae))))
    return ((r - pred) % 256).astype(np.uint8)


def make_log(recon, filtered, bpp, filters):
    h, n = recon.shape
    w = n // bpp
    log = Log()
    _, a, b, c = _neighbours(recon, bpp)
    raw = filtered.astype(np.int64)
    t = np.asarray(filters, np.int64)
    rows = {k: np.flatnonzero(t == k) for k in range(5)}
    log.pred = {(k, bpp): set() for k in range(5) if len(rows[k])}
    for k, pred in ((1, a), (2, b)):
        if len(rows[k]):
            log.pred[(k, bpp)] = {(bool(v),) for v in np.unique(raw[rows[k]] + pred[rows[k]] > 255).tolist()}
    if len(rows[3]):
        s = (a + b)[rows[3]]
        codes = np.unique((s >= 256) * 4 + (s & 1) * 2 + (raw[rows[3]] + (s >> 1) > 255))
        log.pred[(3, bpp)] = {(bool(k & 4), bool(k & 2), bool(k & 1)) for k in codes.tolist()}
    if len(rows[4]):
        log.pred[(4, bpp)] = _paeth_classes(_paeth_parts(a[rows[4]], b[rows[4]], c[rows[4]]))
        top = rows[4][(rows[4] % BAND == 0) & (rows[4] > 0)]
        log.band_top_paeth[bpp] = _paeth_classes(_paeth_parts(a[top], b[top], c[top])) if len(top) else set()
    # positions: of pixels, not bytes
    y, x = np.arange(h, dtype=np.int64)[:, None], np.arange(w, dtype=np.int64)[None, :]
    step = x + y % BAND
    met = {"x=0": x == 0, "y=0": y == 0, "band_top": (y % BAND == 0) & (y > 0), "band_bottom": (y % BAND == BAND - 1) & (y + 1 < h),
           "partial_last": (y == h - 1) & (h % BAND != 0), "x%64=0": x % BAND == 0, "x%64=63": x % BAND == BAND - 1,
           "tile_first": step % BAND == 0, "tile_last": step % BAND == BAND - 1}
    log.positions = {k for k in POSITIONS if np.broadcast_to(met[k], (h, w)).any()}
    log.bands, log.row_bytes = (h + BAND - 1) // BAND, n
    for y0 in range(0, h, BAND):
        last = int(step[y0:y0 + BAND].max())
        log.tiles = max(log.tiles, last // BAND + 1)
        log.last_steps.add(last % BAND)
    return log


def _scanlines(filtered, filters):
    h, n = filtered.shape
    scan = np.zeros((h, n + 1), np.uint8)
    scan[:, 0] = filters
    scan[:, 1:] = filtered
    return scan.tobytes()


def from_filtered(filtered, bpp, filters):
    """-> (scanlines, reconstructed (h, w * bpp) uint8 by the plain un-filter, log)"""
    filtered = np.ascontiguousarray(filtered, np.uint8)
    h, n = filtered.shape
    scan = _scanlines(filtered, filters)
    recon = unfilter(scan, n // bpp, h, bpp)
    return scan, recon, make_log(recon, filtered, bpp, filters)


def from_pixels(pixels, bpp, filters):
    """-> the same; the caller holds the reconstructed image against its pixels (the round trip through the plain un-filter)"""
    return from_filtered(filtered_of(np.ascontiguousarray(pixels, np.uint8), bpp, filters), bpp, filters)


# ---- expansion: include/fpng_amd.h, "Pixels:" ----
BPP = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}


def channels_in_file(color, trns):
    """1, 2, 3 or 4 by colour type; palette: 3, or 4 with a tRNS chunk that holds at least one byte"""
    return {0: 1, 2: 3, 4: 2, 6: 4}[color] if color != 3 else (4 if trns else 3)


def expand(recon, color, plte, trns, desired):
    """recon: (h, w * bpp) uint8; plte: the PLTE chunk that counts (the file's last), trns: the tRNS chunk's bytes, or None each
    -> (h, w, desired) uint8, or ValueError for a palette index at or behind PLTE's entries.  A colour key needs its 2 (grey) or 6
    (RGB) bytes and compares the LOW bytes of its 16-bit samples; palette alpha is read up to 256 bytes, 255 behind tRNS's end."""
    h, n = recon.shape
    bpp = BPP[color]
    px = recon.astype(np.int64).reshape(h, n // bpp, bpp)
    alpha = np.full(px.shape[:2], 255, np.int64)
    trns = bytes(trns) if trns is not None else b""
    if color == 0:
        rgb = np.repeat(px, 3, axis=2)
        if len(trns) >= 2:
            alpha[px[:, :, 0] == trns[1]] = 0
    elif color == 2:
        rgb = px
        if len(trns) >= 6:
            alpha[(px[:, :, 0] == trns[1]) & (px[:, :, 1] == trns[3]) & (px[:, :, 2] == trns[5])] = 0
    elif color == 4:
        rgb, alpha = np.repeat(px[:, :, :1], 3, axis=2), px[:, :, 1]
    elif color == 6:
        rgb, alpha = px[:, :, :3], px[:, :, 3]
    else:
        entries = len(plte) // 3
        if (px >= entries).any():
            raise ValueError("palette index at or behind PLTE's entries")
        table = np.frombuffer(bytes(plte[:3 * entries]), np.uint8).astype(np.int64).reshape(entries, 3)
        table_a = np.full(256, 255, np.int64)
        k = min(len(trns), 256)
        table_a[:k] = np.frombuffer(trns[:k], np.uint8)
        rgb, alpha = table[px[:, :, 0]], table_a[px[:, :, 0]]
    out = np.concatenate([rgb, alpha[:, :, None]], axis=2) if desired == 4 else rgb
    return out.astype(np.uint8)
