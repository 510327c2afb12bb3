"""Which path of walk_row (csrc/kernels.hip) does a row take?  (TEST INFRASTRUCTURE)

A plain numpy restatement of the DECISIONS of the walk's phase A -- the 256-pixel super-windows with four pixels per lane -- and of
nothing else: no tokens, no bits, no sums.  It is used only to PROVE COVERAGE of a list of test images (test_walk_cases_cpu.py:
every tier, row end and flag is reached by some row of the battery), never for an expected byte: the expected files are the
reference's.  An error here can misreport coverage; it cannot make a wrong file pass.

The rules, as in walk_row:
  NS = (w - 1) >> 8 super-windows are followed by a pixel of the row; NSX = NS + 1 when w is a multiple of 256 (the row's last
  super-window is then tried too: `row_end`).
  all_lits: no pixel of the super-window repeats its left neighbour.
  sparse:   some do, rle.carry == 0, no two adjacent repeats (M0 & M1, M1 & M2, M2 & M3, M3 & (M0 >> 1)), and not
            ((M3 >> 63) && next0): the last pixel repeats and the next super-window's first pixel repeats it again.
  else general: replayed as four 64-pixel windows; a row_end super-window is left to phase B instead.
  gen_streak starts at 1, a cheap super-window sets it to 0, a general one adds 1, and at 2 the rest of the row is handed over.
  rle.carry after a sparse super-window is M3 >> 63, after an all-literal one 0, after a 64-pixel window Rle::advance's: the
  leading ones of the window's mask (carry + 64 when all are set) taken mod CAP."""
import os
import re

import numpy as np

from cpu_ref import ROOT

STATES = ("all_lits", "sparse", "general", "handed_over", "row_end_taken", "row_end_left_to_B")
FLAGS = ("carry_nonzero_on_entry", "repeat_on_lane_seam", "repeat_on_super_seam", "next0")


def chunk_cap(c):
    """Rle<C>::CAP, read from the kernels' own constants (csrc/format.h)"""
    with open(os.path.join(ROOT, "fpng_amd", "csrc", "format.h")) as f:
        m = re.search(r"kMaxChunkPixels%d\s*=\s*(\d+)" % c, f.read())
    return int(m.group(1))


def repeats(frow):
    """frow (w, c) filtered pixels -> bool (w,): pixel x equals pixel x - 1 (never pixel 0)"""
    same = np.zeros(len(frow), dtype=bool)
    same[1:] = np.all(frow[1:] == frow[:-1], axis=1)
    return same


def _advance(carry, m, cap):
    """Rle::advance over a 64-pixel window whose repeat flags are m"""
    if m.all():
        t = carry + 64
    else:
        t = 63 - int(np.flatnonzero(~m)[-1])   # leading ones = repeats at the window's end
    return t % cap


def row_path(frow, c):
    """frow (w, c): the FILTERED row -> list, one dict per super-window S < NSX: {"state": one of STATES, and the FLAGS}"""
    w, cap = len(frow), chunk_cap(c)
    same = repeats(frow)
    NS = (w - 1) >> 8
    NSX = NS + (1 if w % 256 == 0 else 0)
    out, carry, gen_streak, limit = [], 0, 1, NSX
    for S in range(NSX):
        m = same[256 * S:256 * S + 256]
        M = [m[j::4] for j in range(4)]
        row_end = S == NS
        next0 = (not row_end) and bool(same[256 * (S + 1)])
        rec = {"carry_nonzero_on_entry": carry != 0, "repeat_on_lane_seam": bool(M[0].any()),
               "repeat_on_super_seam": S > 0 and bool(m[0]), "next0": next0}
        if S >= limit:
            rec["state"] = "handed_over"
            out.append(rec)
            continue
        all_lits = not m.any()
        adjacent = (M[0] & M[1]).any() or (M[1] & M[2]).any() or (M[2] & M[3]).any() or (M[3][:-1] & M[0][1:]).any()
        sparse = (not all_lits) and carry == 0 and not adjacent and not (m[255] and next0)
        if all_lits or sparse:
            gen_streak = 0
            rec["state"] = "row_end_taken" if row_end else ("sparse" if sparse else "all_lits")
            rec["tier"] = "sparse" if sparse else "all_lits"
            carry = int(m[255]) if sparse else 0
        elif row_end:
            rec["state"] = "row_end_left_to_B"
            limit = S
        else:
            rec["state"] = "general"
            gen_streak += 1
            for jw in range(4):
                carry = _advance(carry, m[64 * jw:64 * jw + 64], cap)
            if gen_streak >= 2:
                limit = S + 1
        out.append(rec)
    return out


def image_paths(img):
    """img (h, w, c) -> one row_path per row, of the rows as the encoder filters them (row 0 as it is, Up below)"""
    f = img.copy()
    f[1:] = img[1:] - img[:-1]
    return [row_path(f[y], img.shape[2]) for y in range(img.shape[0])]
