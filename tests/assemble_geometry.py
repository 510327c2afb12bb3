"""The encoder's CRC / assembly geometry restated in Python from the comment of fpng_amd/csrc/crc_geometry.h (TEST INFRASTRUCTURE).

How scan_kernel, assemble_kernel (or the stored_* kernels) and finalize_kernel divide a file depends on the file's size, the number
of jobs of the submission and the image's maximum size, never on its content:

  data_end = 58 + zlib_size - 4 = file size - 20;  end_aligned = round_up(data_end, 16);  pad = end_aligned - data_end
  span = 58 + zlib_size = file size - 16;  want = max(4, 2048 // n_jobs);  crc_blocks = ceil(max encoded size / 64 KiB) + 1
  rl = the least of 12 .. 16 with (span >> rl) + 1 <= min(want, crc_blocks), else 16
  n_ranges = ceil((end_aligned - 48) / 2^rl);  sliver = (end_aligned - 48) mod 2^rl (the farthest range's bytes, 0 = a full one)
  g = the least with 256 * 2^g >= n_ranges;  fold rows rl - 12 (columns < 2^g) and rl + g - 12 (columns < 256) of fold[13][256]

The ranges, the 4 KiB rows inside them and the 16-byte pieces all hang off end_aligned.  A stored file's zlib stream is 78 01, then
blocks of 65535 stream bytes behind 5-byte headers, at file offsets 60 + 65540 k."""
from collections import namedtuple

import numpy as np

HEAD, TAIL, FIRST_PIECE = 58, 16, 48
STORED_MAX, STORED_PERIOD = 65535, 65540
ROW_BYTES = 4096
FOLD_ROWS, FOLD_COLS, FOLD_THREADS = 13, 256, 256

Geometry = namedtuple("Geometry", "rl n_ranges g pad sliver")


def n_filtered(w, h, c):
    return (w * c + 1) * h


def stored_blocks(w, h, c):
    return (n_filtered(w, h, c) + STORED_MAX - 1) // STORED_MAX


def max_encoded_size(w, h, c):
    n = n_filtered(w, h, c)
    return HEAD + 6 + n + 5 * stored_blocks(w, h, c) + TAIL


def crc_blocks(w, h, c):
    return (max_encoded_size(w, h, c) + 65535) // 65536 + 1


def stored_size(w, h, c):
    """the size of the file of stored blocks (flags = 2, or what does not compress): a closed form of the dimensions"""
    return max_encoded_size(w, h, c)


def want_of(n_jobs):
    return max(4, 2048 // n_jobs)


def range_log2(span, n_jobs, blocks):
    rl = 12
    while rl < 16 and ((span >> rl) + 1 > want_of(n_jobs) or (span >> rl) + 1 > blocks):
        rl += 1
    return rl


def end_aligned_of(size):
    return (size - 20 + 15) & ~15


def rule(span, n_jobs, blocks):
    """(rl, n_ranges, g, pad, sliver, fold step row, fold group row) of a file of span + 16 bytes"""
    rl = range_log2(span, n_jobs, blocks)
    data_end = span - 4
    ea = (data_end + 15) & ~15
    n = (ea - FIRST_PIECE + (1 << rl) - 1) >> rl
    g = 0
    while (FOLD_THREADS << g) < n:
        g += 1
    return rl, n, g, ea - data_end, (ea - FIRST_PIECE) & ((1 << rl) - 1), rl - 12, rl + g - 12


def geometry(w, h, c, size, n_jobs):
    return Geometry(*rule(size - TAIL, n_jobs, crc_blocks(w, h, c))[:5])


def cell_of(w, h, c, size, n_jobs):
    """what a case of tests/golden/geometry.json records of its geometry"""
    return dict(geometry(w, h, c, size, n_jobs)._asdict())


def _straddles(off, length, end_aligned, period):
    """does [off, off + length) hold a boundary of the grid of `period` bytes that hangs off end_aligned in its inside?"""
    return (end_aligned - off) % period < length and (end_aligned - off) % period != 0


def stored_walk(w, h, c, n_jobs=1):
    """Where a stored file's block headers and filter bytes lie against the pieces, 4 KiB rows and ranges.
    -> dict: geometry; headers: per block (file offset, offset in its piece, straddles a piece / a row / a range boundary);
       filters: per image row the filter byte's file offset and its offset in its piece, its 4 KiB row and its range;
       filter_piece_offsets: the set of the offsets in a piece;  pieces: what the fast path of assemble_stored takes (stored_pieces)"""
    size = stored_size(w, h, c)
    geo = geometry(w, h, c, size, n_jobs)
    ea = end_aligned_of(size)
    headers = []
    for k in range(stored_blocks(w, h, c)):
        off = 60 + STORED_PERIOD * k
        headers.append(dict(block=k, offset=off, in_piece=off % 16, straddles_piece=off % 16 > 11, straddles_row=_straddles(off, 5, ea, ROW_BYTES),
                            straddles_range=_straddles(off, 5, ea, 1 << geo.rl)))
    stride = w * c + 1
    s = np.arange(h, dtype=np.int64) * stride
    fo = 65 + 5 * (s // STORED_MAX) + s
    filters = dict(offset=fo, in_piece=fo % 16, in_row=(fo - ea) % ROW_BYTES, in_range=(fo - ea) % (1 << geo.rl))  # arrays, one entry per row
    return dict(size=size, geometry=geo, end_aligned=ea, headers=headers, filters=filters, filter_piece_offsets=sorted(set((fo % 16).tolist())),
                pieces=stored_pieces(w, h, c))


def stored_pieces(w, h, c):
    """assemble_stored's fast path (16 consecutive pixel bytes of one row and one block, loaded as dwords) over every piece of the file,
    for a source whose first byte is 4-byte aligned: -> dict of the number of fast pieces, of those with col == 1, with
    col + 16 == stride, per source misalignment m, and whether the piece with the image's last 16 bytes is a fast one"""
    stride, bpl = w * c + 1, w * c
    nf = stride * h
    ea = end_aligned_of(stored_size(w, h, c))
    fo = np.arange(64, ea, 16, dtype=np.int64)
    z = fo - HEAD
    k, wq = (z - 2) // STORED_PERIOD, (z - 2) % STORED_PERIOD
    s0 = k * STORED_MAX + (wq - 5)
    ok = (wq >= 5) & (wq <= STORED_PERIOD - 16) & (s0 + 16 <= nf)
    r, col = s0 // stride, s0 % stride
    fast = ok & (col >= 1) & (col + 16 <= stride)
    m = (r * bpl + col - 1) & 3
    return dict(fast=int(fast.sum()), col1=int((fast & (col == 1)).sum()), col_end=int((fast & (col + 16 == stride)).sum()),
                m=[int((fast & (m == q)).sum()) for q in range(4)], last16=bool((fast & (s0 + 16 == nf)).any()))


def header_class(w, h, c, block=4, n_jobs=1):
    """'piece', 'row' or 'range': the coarsest boundary that the header of stored block `block` straddles (None: the file has no such block)"""
    hd = stored_walk(w, h, c, n_jobs)["headers"]
    if block >= len(hd):
        return None
    e = hd[block]
    return "range" if e["straddles_range"] else "row" if e["straddles_row"] else "piece" if e["straddles_piece"] else "none"


# ---------------------------------------------------------------------------------------------
# The images of tests/golden/geometry.json (oracle/make_golden_geometry.py finds the cases, test_gpu_encode_geometry.py runs them)
# ---------------------------------------------------------------------------------------------
GROUP_A_JOBS = 528  # the jobs of each of group A's submissions (one per mode): 2048 // 528 < 4, so want = 4 binds


def case_image(w, h, c, seed, noise_pixels):
    """zeros whose first noise_pixels pixels in row-major order are fpng_amd.synth_image's noise of that seed (a prefix of one stream:
    one more pixel changes nothing in front of it) -> uint8 (h, w, c)"""
    import fpng_amd
    img = np.zeros((h * w, c), dtype=np.uint8)
    if noise_pixels:
        img[:noise_pixels] = fpng_amd.synth_image("noise", noise_pixels, 1, c, seed=seed).reshape(noise_pixels, c)
    return img.reshape(h, w, c)


def filler(flags, i):
    """job i of the distinct small jobs that fill a group A submission up to GROUP_A_JOBS: (w, h, c, seed, noise_pixels).  Compressed
    modes: raw images a little over 192 KiB (crc_blocks = 5) whose files spread from 2 KB to 150 KB; stored: small images of many shapes"""
    if flags & 2:
        w, h, c = 1 + (i * 7) % 300, 1 + (i * 13) % 200, 3 + (i & 1)
        return w, h, c, 5000 + i, w * h
    w, h, c = (256, 192, 4) if i & 1 else (256, 257, 3)
    return w, h, c, 5000 + i, 50 + (i * 97) % 30000  # (never 0: zeros are one image whatever the seed)
