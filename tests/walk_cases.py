"""The row walk's case battery (TEST INFRASTRUCTURE, numpy only): the generators of test_gpu_parity's walk tests -- super-window
tiers, row ends, window / chunk widths, runs across 256-pixel borders, the wide fuzz -- in one place, `layout_battery(c)`: a fixed
list of small images built from them for the walks of the OTHER source layouts (test_gpu_layout_walk.py), and the byte layouts
those sources are handed over in.  Patterns are built on the FILTERED rows and integrated over y (pixel = up + filtered mod 256), so
that the Up filter gives the pattern back on every row; row 0 is filtered as it stands.  tests/walk_tier_model.py says which path
of walk_row a row takes; test_walk_cases_cpu.py holds the battery to every one of them."""
import importlib.util
import os

import numpy as np

from cpu_ref import ROOT

TIER_KINDS = ("sparse", "lit_then_runs", "runs_then_lit", "alternate", "pairs", "long_run_mid")
NEW_TIER_KINDS = ("seam_repeats", "carry_in")
ROW_ENDS = ("literal", "repeat1", "repeat2", "run_cap", "solid_tail", "sparse")
WINDOW_KINDS = ("solid", "runs40", "filtered_runs", "alternation")

# what a seam_repeats row adds to its isolated repeats, by variant (= the row's y in the battery): a repeat in the last pixel of a
# super-window with and without one in the first pixel of the next (M3 >> 63 with next0 false / true), the seam alone, a pair
# inside one lane (M0 & M1) and one across two lanes (M3 & (M0 >> 1))
_SEAMS = ((255,), (256, 512), (255, 256), (256, 257, 511), (259, 260, 512))


def _isolated(w, variant, skip):
    """positions 4k + j, 12 pixels apart, j cycling over the four places of a lane, none within 3 pixels of `skip`"""
    xs = []
    for i, k in enumerate(range(2, w // 4, 3)):
        x = 4 * k + (0, 1, 3, 2)[(i + variant) % 4]
        if x < w and all(abs(x - s) > 3 for s in skip):
            xs.append(x)
    return xs


def tier_pattern(rng, kind, w, c, variant=0):
    """One FILTERED row exercising a particular mix of the row walker's super-window (256 px) tiers."""
    row = rng.integers(0, 256, (w, c), dtype=np.uint8)
    x = np.arange(w)
    if kind == "sparse":           # isolated repeats, some of them straddling 4-pixel lane groups and super-window seams
        rep = rng.random(w) < 0.01
        rep[[i for i in (1, 3, 4, 255, 256, 257, 511, 512) if i < w]] = True
        rep[0] = False
        for i in np.flatnonzero(rep):
            row[i] = row[i - 1]
    elif kind == "lit_then_runs":  # literal super-windows, then run-heavy ones (walker hands the row over mid-way)
        row[x >= (w // 2)] = row[w // 2]
    elif kind == "runs_then_lit":
        row[x < (w // 2)] = 9
    elif kind == "alternate":      # general and literal super-windows alternate: the hand-over streak must reset
        for s in range(0, w, 512):
            row[s:s + 200] = row[s]
    elif kind == "pairs":          # every second pixel repeats: 1-pixel matches everywhere (literal-vs-match rule)
        row[1::2] = row[0:w - (w % 2):2][: len(row[1::2])]
    elif kind == "long_run_mid":   # a run longer than the chunk cap crossing several super-windows
        a, b = w // 5, w - w // 7
        row[a:b] = row[a]
    elif kind == "seam_repeats":   # literals, isolated repeats in every place of a lane, and the variant's repeats at the seams
        seams = [s for s in _SEAMS[variant % len(_SEAMS)] if s < w]
        for i in sorted(set(_isolated(w, variant, (255, 256, 257, 259, 260, 511, 512))) | set(seams)):
            row[i] = row[i - 1]
    elif kind == "carry_in":       # a sparse super-window whose last pixel repeats, then an all-literal one (odd variants: one
        xs = [i for i in _isolated(w, variant, (255,)) if i < 250 or i >= 512]    # isolated repeat in it), then sparse ones
        xs += [255] + ([300] if variant & 1 else [])
        for i in sorted(i for i in xs if 0 < i < w):
            row[i] = row[i - 1]
    return row


def integrate(rows):
    """filtered rows (h, w, c) -> the image whose Up filter gives them back"""
    return np.ascontiguousarray(np.cumsum(rows.astype(np.uint16), axis=0).astype(np.uint8))


def window_chunk_image(rng, kind, w, h, c):
    """The four contents of the window (64 px) / chunk-cap (63 / 85 px) width test"""
    if kind == 0:      # solid
        img = np.full((h, w, c), 77, dtype=np.uint8)
    elif kind == 1:    # long runs with random breaks
        img = np.repeat(rng.integers(0, 256, (h, (w + 39) // 40, c), dtype=np.uint8), 40, axis=1)[:, :w]
    elif kind == 2:    # runs of random length 1..200 on the FILTERED rows: make rows identical so Up gives zeros after row 0
        row = np.repeat(rng.integers(0, 256, (1, w, c), dtype=np.uint8), h, axis=0)
        brk = rng.random((1, w)) < 0.03
        row[:, ~brk[0]] = 0
        row = np.maximum.accumulate(row, axis=1)
        img = row
    else:              # two-pixel alternation (1-pixel matches -> literal-vs-match rule)
        a = rng.integers(0, 256, (h, 1, c), dtype=np.uint8)
        img = np.repeat(a, w, axis=1).copy()
        img[:, 2::3] = rng.integers(0, 256, (h, len(range(2, w, 3)), c), dtype=np.uint8)
    return np.ascontiguousarray(img)


def window_chunk_cases(c):
    """test_widths_around_window_and_chunk_limits' list -> (images, (w, h, c) of each)"""
    rng = np.random.default_rng(7 + c)
    imgs, dims = [], []
    for w in [1, 2, 3, 62, 63, 64, 65, 66, 84, 85, 86, 87, 126, 127, 128, 129, 130, 170, 171, 172, 191, 192, 193, 255, 256,
              257, 500, 1000, 4099]:
        for h in (1, 2, 5):
            for kind in range(4):
                imgs.append(window_chunk_image(rng, kind, w, h, c))
                dims.append((w, h, c))
    return imgs, dims


def super_window_tier_cases(c):
    """test_super_window_tiers' list -> (images, (w, h, c) of each)"""
    rng = np.random.default_rng(40 + c)
    imgs, dims = [], []
    for w in [252, 256, 257, 259, 260, 511, 512, 513, 516, 768, 1023, 1024, 1025, 1300, 2065]:
        for kind in TIER_KINDS:
            r0 = tier_pattern(rng, kind, w, c)
            r1 = (r0.astype(np.uint16) + tier_pattern(rng, kind, w, c)).astype(np.uint8)   # Up-filtered row 1 = second pattern
            r2 = (r1.astype(np.uint16) + tier_pattern(rng, "sparse", w, c)).astype(np.uint8)
            imgs.append(np.ascontiguousarray(np.stack([r0, r1, r2])))
            dims.append((w, 3, c))
    return imgs, dims


def row_end_image(rng, end, w, c, h=3):
    """Rows of at least 256 pixels with one kind of row end: literal, isolated repeat, run into the last pixel, run through the
    whole last super-window"""
    rows = rng.integers(0, 256, (h, w, c), dtype=np.uint8)
    for r in rows:  # the FILTERED rows get the pattern: build them, then integrate over y
        if end == "repeat1":
            r[w - 1] = r[w - 2]
        elif end == "repeat2":
            r[w - 2:] = r[w - 3]
        elif end == "run_cap":
            r[w - 64:] = r[w - 65]
        elif end == "solid_tail":
            r[w - 256:] = 5
        elif end == "sparse":
            for i in (3, 64, 200, w - 5, w - 1):
                r[i] = r[i - 1]
    return np.ascontiguousarray(np.cumsum(rows.astype(np.uint16), axis=0).astype(np.uint8))


def row_end_cases(c):
    """test_rows_ending_on_a_super_window's list -> (end, w, image) in the test's order"""
    rng = np.random.default_rng(90 + c)
    return [(end, w, row_end_image(rng, end, w, c))
            for w in (256, 257, 259, 300, 511, 512, 700, 768, 1000, 1024, 1920, 3840, 4099)   # the last super-window complete or partial
            for end in ROW_ENDS]


def direct_cases(rng):
    """Images that put seams where they hurt a walk in 256-pixel steps: widths just over / under / on multiples of 256, runs that cross seams or end
    on them, flat rows (one run over the whole row: the look back over the pixels in front of a piece walks to the row's start),
    64-pixel tiles, noise (chunks that overflow the wave's window and spill), gradients."""
    import fpng_amd
    cases = []
    for w in (257, 300, 511, 512, 513, 768, 1025, 1280, 1537, 2049, 2304):
        for c in (3, 4):
            h = int(rng.integers(3, 12))
            for kind in ("grad", "blocks", "solid"):
                cases.append((fpng_amd.synth_image(kind, w, h, c, seed=int(rng.integers(1, 1 << 30))), w, h, c))
            # runs of random lengths (1..700 pixels) of random colours, rows repeated now and then (Up-filtered: all-zero rows)
            img = np.zeros((h, w, c), dtype=np.uint8)
            for y in range(h):
                if y and rng.random() < 0.3:
                    img[y] = img[y - 1]
                    continue
                x = 0
                while x < w:
                    n = int(rng.integers(1, 700)) if rng.random() < 0.5 else int(rng.integers(1, 6))
                    img[y, x:x + n] = rng.integers(0, 256, c, dtype=np.uint8)
                    x += n
            cases.append((img, w, h, c))
            # a run that ends exactly on / one pixel after / one before every multiple of 256
            img = rng.integers(0, 256, (h, w, c), dtype=np.uint8)
            for y in range(h):
                for s0 in range(256, w, 256):
                    e = s0 + int(rng.integers(-1, 2))
                    b = max(0, e - int(rng.integers(2, 200)))
                    img[y, b:e] = img[y, b]
            cases.append((img, w, h, c))
    cases.append((fpng_amd.synth_image("noise", 2048, 5, 4), 2048, 5, 4))
    cases.append((fpng_amd.synth_image("noise", 3000, 4, 3), 3000, 4, 3))
    return cases


_wide = None


def wide_fuzz():
    """tools/gpu_wide_fuzz.py as a module (its wide_image is the generator)"""
    global _wide
    if _wide is None:
        spec = importlib.util.spec_from_file_location("gpu_wide_fuzz", os.path.join(ROOT, "tools", "gpu_wide_fuzz.py"))
        _wide = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(_wide)
    return _wide


# ---------------------------------------------------------------------------------------------
# the battery
# ---------------------------------------------------------------------------------------------
BATTERY_H = 5
BATTERY_MAX_W = 2065
TIER_WIDTHS = (256, 257, 259, 260, 511, 512, 513, 516, 768, 1023, 1024, 1025, 1300, 2065)
ROW_END_WIDTHS = (256, 257, 259, 300, 511, 512, 768, 1024, 1920)
SHORT_WIDTHS = (1, 2, 3, 62, 63, 64, 65, 66, 85, 86, 127, 128, 129, 130, 191, 193, 253, 254, 255)
N_WIDE = 60
_battery = {}


def layout_battery(c):
    """-> [(name, image (h, w, c))]: about 300 seeded images of at most 2065 x 5 pixels, the same list on every call.  Names start
    with the group: tier / end / short / wide."""
    if c in _battery:
        return _battery[c]
    rng = np.random.default_rng([20260, c])
    out = []
    for w in TIER_WIDTHS:
        for kind in TIER_KINDS + NEW_TIER_KINDS:
            rows = np.stack([tier_pattern(rng, kind, w, c, variant=y) for y in range(BATTERY_H)])
            out.append((f"tier {kind} {w}", integrate(rows)))
    for w in ROW_END_WIDTHS:
        for end in ROW_ENDS:
            out.append((f"end {end} {w}", row_end_image(rng, end, w, c, BATTERY_H)))
    for w in SHORT_WIDTHS:
        for kind in range(4):
            out.append((f"short {WINDOW_KINDS[kind]} {w}", window_chunk_image(rng, kind, w, BATTERY_H, c)))
    # the wide fuzz draws c, w (up to 4100) and h (up to 6) itself: its images of this c that fit the battery's bounds, in order
    frng, n = np.random.default_rng([4000, c]), 0
    while n < N_WIDE:
        img, w, h, cc = wide_fuzz().wide_image(frng)
        if cc == c and w <= BATTERY_MAX_W and h <= BATTERY_H:
            out.append((f"wide {n} {w}x{h}", img))
            n += 1
    for _, img in out:
        img.setflags(write=False)
    _battery[c] = out
    return out


# ---------------------------------------------------------------------------------------------
# source layouts: where the bytes (or elements) of an image lie in the buffer a submission points into
# ---------------------------------------------------------------------------------------------
PLANAR_KINDS = ("odd", "neg", "rev", "far", "3of4", "phases")


def planes(vals, kind, fill=None):
    """Lays vals (h, w, c) -- bytes, or the bits of 16- / 32-bit elements -- out as planes in one flat buffer of the same type ->
    (buffer, element offset of plane 0's top row, row pitch, plane pitch; both in elements).  kind: test_gpu_planar's contig | wide |
    odd | neg | rev | far (4099 elements here) | 3of4, and phases: base 1, row pitch = 1 and plane pitch = 3 (mod 4), so that the planes of one image start
    at four different bytes mod 4 and a row and the row above never share a phase.  Everything that is not a pixel comes from `fill`
    (a generator), or is zero."""
    h, w, c = vals.shape
    slots = 4 if kind == "3of4" else c
    if kind == "phases":
        ap = w + (1 - w) % 4
        app = h * ap + (3 - h * ap) % 4
        front = 1
    else:
        ap = w + {"wide": 256, "odd": 1, "neg": 8}.get(kind, 0)
        app = h * ap + {"odd": 3, "rev": 5, "far": 4099}.get(kind, 0)
        front = 1 if kind == "odd" else 16
    total = front + slots * app + 16
    if fill is None:
        buf = np.zeros(total, dtype=vals.dtype)
    else:
        buf = fill.integers(0, 1 << (8 * vals.itemsize), total, dtype=np.uint64).astype(vals.dtype)

    def off(ch, r):
        return front + ((c - 1 - ch) if kind == "rev" else ch) * app + ((h - 1 - r) if kind == "neg" else r) * ap
    for ch in range(c):
        for r in range(h):
            buf[off(ch, r):off(ch, r) + w] = vals[r, :, ch]
    return buf, off(0, 0), (-ap if kind == "neg" else ap), (-app if kind == "rev" else app)


def plane_row_offsets(top, rp, pp, h, c):
    """element offsets of the first element of row r of plane ch -> array (c, h)"""
    return top + pp * np.arange(c)[:, None] + rp * np.arange(h)[None, :]


EX_FORMATS = ("RGB", "BGR", "BGRA", "ABGR", "RGBX", "XBGR")


def ex_pitch_kind(i, sb):
    kinds = ("packed", "wide", "neg") + (("odd",) if sb == 3 else ())
    return kinds[i % len(kinds)]


# float sources whose quantisation is exact by construction: element = byte, or element = byte - 128 with a bias of 128
FLOAT_SETS = {"plain": (0.0, 1.0, 0.0), "biased": (-128.0, 1.0, 128.0)}   # name -> (added to the byte, scale, bias)
NP_BITS = {0: np.uint32, 1: np.uint16, 2: np.uint16}   # FPNG_AMD_F32 / _F16 / _BF16


def float_table(code, add):
    """the 256 elements (as stored bits) that stand for the bytes 0 .. 255 in a float source: byte + add in the dtype `code`"""
    from test_float_encode_cpu import to_elements
    return np.ascontiguousarray(to_elements(np.arange(256, dtype=np.float64) + add, code)).view(NP_BITS[code])


def float_bits(img, code, add):
    """img (h, w, c) bytes -> the bits of its float elements, every one an entry of float_table"""
    return float_table(code, add)[img]


def planar_kind(i, c):
    kinds = [k for k in PLANAR_KINDS if not (k == "3of4" and c == 4)]
    return kinds[i % len(kinds)]
