"""No-GPU tests of the row walk's case battery (tests/walk_cases.py), which test_gpu_layout_walk.py sends through every source
layout's instantiation of walk_row:

  coverage     per tests/walk_tier_model.py, the battery reaches every path of the walk's phase A -- tier, row end, hand-over, with and
               without a row above -- and every flag, width residue and tier change the walk branches on;
  sensitivity  deliberately wrong MODELS of the layouts' loads (never a wrong kernel): each changes the reference's file for some
               battery image of every layout it could occur in, so the GPU test would see it;
  exactness    the float sources' elements quantise back to the bytes they stand for, all of them, in all three dtypes.
"""
import numpy as np
import pytest

import walk_cases as W
import walk_tier_model as M
from cpu_ref import have_ref, oracle, ref
from test_float_encode_cpu import element_values, oracle_quantize


def _judge(img, flags=0):
    h, w, c = img.shape
    return (ref() if have_ref() else oracle()).encode(np.ascontiguousarray(img), w, h, c, flags)


@pytest.fixture(scope="module")
def paths():
    """c -> [(name, image, image_paths)]"""
    return {c: [(name, img, M.image_paths(img)) for name, img in W.layout_battery(c)] for c in (3, 4)}


def test_battery_is_fixed_and_small():
    for c in (3, 4):
        a = W.layout_battery(c)
        W._battery.pop(c)
        b = W.layout_battery(c)
        assert len(a) == len(b) and all(x[0] == y[0] and np.array_equal(x[1], y[1]) for x, y in zip(a, b))
        assert 280 <= len(a) <= 320
        assert all(i.shape[2] == c and i.shape[1] <= W.BATTERY_MAX_W and i.shape[0] <= W.BATTERY_H for _, i in a)
        assert len({n for n, _ in a}) == len(a)


def test_model_constants_and_rules():
    assert M.chunk_cap(3) == 85 and M.chunk_cap(4) == 63
    rng = np.random.default_rng(1)
    lit = rng.integers(0, 256, (1024, 3), dtype=np.uint8)
    lit[1:][np.all(lit[1:] == lit[:-1], axis=1), 0] ^= 1
    assert [r["state"] for r in M.row_path(lit, 3)] == ["all_lits"] * 3 + ["row_end_taken"]
    assert M.row_path(lit[:1023], 3)[-1]["state"] == "all_lits" and len(M.row_path(lit[:1023], 3)) == 3
    assert M.row_path(lit[:255], 3) == [] and len(M.row_path(lit[:257], 3)) == 1
    r = lit.copy()
    r[255] = r[254]                       # the last pixel of super-window 0 repeats: sparse, and the carry goes into the next one
    p = M.row_path(r, 3)
    assert (p[0]["state"], p[1]["state"], p[1]["carry_nonzero_on_entry"]) == ("sparse", "all_lits", True)
    r[256] = r[255]                       # ... and the next one repeats it again: super-window 0 is general, the row handed over at once
    assert [q["state"] for q in M.row_path(r, 3)] == ["general", "handed_over", "handed_over", "handed_over"]
    r = lit.copy()
    r[300:400] = r[300]                   # 99 repeats end inside super-window 1: general once, then cheap again
    assert [q["state"] for q in M.row_path(r, 3)] == ["all_lits", "general", "all_lits", "row_end_taken"]
    r[1000:] = r[1000]
    assert M.row_path(r, 3)[-1]["state"] == "row_end_left_to_B"
    r = lit.copy()
    r[300:768] = r[300]                   # a run through super-windows 1 and 2: 211 repeats in front of the seam, carried mod CAP
    p = M.row_path(r, 3)
    assert [q["state"] for q in p] == ["all_lits", "general", "general", "handed_over"]
    assert p[2]["carry_nonzero_on_entry"] and p[2]["repeat_on_super_seam"] and p[1]["next0"] and not p[1]["repeat_on_super_seam"]
    r = lit.copy()
    r[341:512] = r[341]                   # 170 = 2 * CAP repeats in front of the seam: the carry is 0 again
    assert not M.row_path(r, 3)[2]["carry_nonzero_on_entry"] and M.row_path(r, 4)[2]["carry_nonzero_on_entry"]


@pytest.mark.parametrize("c", [3, 4])
def test_coverage(paths, c):
    """every cell of {state} x {row 0, rows 1 ...}, every flag both ways, the width residues, the tier changes: printed, none empty"""
    cells = {(s, top): 0 for s in M.STATES for top in (True, False)}
    flags = {(f, v): 0 for f in M.FLAGS for v in (True, False)}
    sgs = handed_mid = 0
    for name, img, rows in paths[c]:
        for y, row in enumerate(rows):
            states = [r["state"] for r in row]
            for r in row:
                cells[(r["state"], y == 0)] += 1
                for f in M.FLAGS:
                    flags[(f, r[f])] += 1
            sgs += any(states[i:i + 3] == ["sparse", "general", "sparse"] for i in range(len(states) - 2))
            handed_mid += "handed_over" in states and states.index("handed_over") >= 2
    print(f"\nC = {c}: super-windows of the battery by path (row 0 / rows 1 ...)")
    for s in M.STATES:
        print(f"  {s:18s} {cells[(s, True)]:6d} {cells[(s, False)]:6d}")
    for f in M.FLAGS:
        print(f"  {f:24s} true {flags[(f, True)]:6d}  false {flags[(f, False)]:6d}")
    print(f"  rows with sparse -> general -> sparse: {sgs};  rows handed over behind two or more super-windows: {handed_mid}")
    short_w = {img.shape[1] for name, img, _ in paths[c] if name.startswith("short")}
    all_w = {img.shape[1] for _, img, _ in paths[c]}
    print(f"  short rows' w % 4: {sorted({w % 4 for w in short_w})};  w % 256 of all rows: {sorted({w % 256 for w in all_w})}")
    empty = [k for k, v in {**cells, **flags}.items() if v == 0]
    assert not empty, f"no battery row reaches {empty}"
    assert {w % 4 for w in short_w} == {0, 1, 2, 3} and max(short_w) < 256
    assert {0, 1, 3, 4, 255} <= {w % 256 for w in all_w if w >= 255}
    assert sgs > 0 and handed_mid > 0   # (a `handed_over` entry IS a super-window behind the hand-over; index >= 2: in mid-row)


# ---------------------------------------------------------------------------------------------
# sensitivity: wrong models of the loads
# ---------------------------------------------------------------------------------------------
def _phase_a_spans(rows_paths, y):
    """pixel ranges of row y that phase A's four-pixels-per-lane code sees (every super-window it classifies)"""
    return [(256 * S, 256 * S + 256) for S, r in enumerate(rows_paths[y]) if r["state"] not in ("handed_over",)]


def _fault_swap(img, rows_paths, plane):
    """pixels 1 and 2 of every lane group swapped in one plane (all planes: plane = None), where phase A runs"""
    out = img.copy()
    for y in range(img.shape[0]):
        for a, b in _phase_a_spans(rows_paths, y):
            seg = out[y, a:b].reshape(64, 4, -1)
            ch = slice(None) if plane is None else plane
            seg[:, [1, 2], ch] = seg[:, [2, 1], ch]
    return out


def _fault_seam_compare(img, rows_paths):
    """the first pixel of a super-window from 1 on compared with the wrong predecessor = its repeat flag forced off: the pixels a
    decoder would get from such a file's tokens are those of an image whose pixel 256 k does not repeat -- modelled by making it
    differ, where it did repeat and phase A looks at it"""
    out = img.copy()
    f = img.copy()
    f[1:] = img[1:] - img[:-1]
    for y in range(img.shape[0]):
        same = M.repeats(f[y])
        for a, b in _phase_a_spans(rows_paths, y):
            if a and same[a]:
                out[y, a, 0] += 1
    return out


def _planar_buffers(img, i, c, code=None, add=0.0):
    """the source buffer of battery image i as the GPU test lays it out (bytes, or float bits) + offsets of (plane, row)"""
    vals = img if code is None else W.float_bits(img, code, add)
    buf, top, rp, pp = W.planes(vals, W.planar_kind(i, c), np.random.default_rng(i))
    return buf, W.plane_row_offsets(top, rp, pp, img.shape[0], c)


def _to_bytes(bits, code, add):
    if code is None:
        return bits
    scale, bias = 1.0, -add
    return oracle_quantize(element_values(bits.view({0: np.float32, 1: np.float16, 2: np.uint16}[code]), code), scale, bias)


def _fault_phase3_shift(img, i, c, plane=0):
    """one plane's rows read one byte late where the row starts at phase 3 (planar bytes)"""
    buf, offs = _planar_buffers(img, i, c)
    out = img.copy()
    for y in range(img.shape[0]):
        o = int(offs[plane, y])
        if o % 4 == 3:
            out[y, :, plane] = buf[o + 1:o + 1 + img.shape[1]]
    return out


def _fault_phase3_shift_ex(img, i, name):
    """a 3-byte packed row read one byte late where it starts at phase 3"""
    from test_gpu_layouts import _layout, _to_source
    h, w, _ = img.shape
    src = _to_source(img, name, None)
    buf, top, pitch = _layout(src, W.ex_pitch_kind(i, 3), np.random.default_rng(i))
    out = img.copy()
    for y in range(h):
        o = top + y * pitch
        if o % 4 == 3:
            got = buf[o + 1:o + 1 + 3 * w].reshape(w, 3)
            for k, ch in enumerate(name):
                out[y, :, "RGB".index(ch)] = got[:, k]
    return out


def _fault_past_the_end(img, i, c, code=None, add=0.0, plane=0):
    """the element just past the row's end taken for the last pixel's, where the row does not end on a lane group"""
    h, w, _ = img.shape
    if w % 4 == 0:
        return img
    buf, offs = _planar_buffers(img, i, c, code, add)
    out = img.copy()
    for y in range(h):
        o = int(offs[plane, y])
        out[y, w - 1, plane] = _to_bytes(buf[o + w:o + w + 1], code, add)[0]
    return out


def _first_seen(battery, fault):
    """the first battery image whose pixels the fault changes -> (name, files differ)"""
    for i, (name, img, rows_paths) in enumerate(battery):
        bad = fault(i, img, rows_paths)
        if not np.array_equal(bad, img):
            return name, _judge(bad) != _judge(img)
    return None, False


@pytest.mark.parametrize("c", [3, 4])
def test_wrong_load_models_change_the_file(paths, c):
    """For every layout a fault could occur in, some battery image's file changes under it.  (The 13 layouts: packed C3 / C4, _ex
    RGB BGR | RGBX XBGR | BGRA ABGR, planar bytes, planar f32 / f16 / bf16.)"""
    battery = paths[c]
    planar_like = [("planar", None, 0.0)] + [(f"float{code} {s}", code, add) for code in (0, 1, 2) for s, (add, _, _) in W.FLOAT_SETS.items()]
    seen = {}
    # 1. pixels 1 and 2 of a lane group swapped: one plane of a planar source (every plane), whole pixels of a packed one
    for plane in range(c):
        seen[f"swap 1<->2, plane {plane} (planar, float)"] = _first_seen(battery, lambda i, img, rp: _fault_swap(img, rp, plane))
    seen["swap 1<->2, pixels (packed, _ex)"] = _first_seen(battery, lambda i, img, rp: _fault_swap(img, rp, None))
    # 2. rows at byte phase 3 read one byte late: planar bytes (per plane), 3-byte _ex sources
    for plane in range(c):
        seen[f"phase 3 one byte late, planar plane {plane}"] = _first_seen(battery, lambda i, img, rp: _fault_phase3_shift(img, i, c, plane))
    if c == 3:
        for name in ("RGB", "BGR"):
            seen[f"phase 3 one byte late, {name}"] = _first_seen(battery, lambda i, img, rp: _fault_phase3_shift_ex(img, i, name))
    # 3. the element past the row's end in the last pixel: sources whose resources end on a dword (planar, float)
    for what, code, add in planar_like:
        for plane in range(c):
            seen[f"past the end, {what} plane {plane}"] = _first_seen(battery, lambda i, img, rp: _fault_past_the_end(img, i, c, code, add, plane))
    # 4. the seam compare: every layout shares the battery's pixels
    seen["seam compare (all 13 layouts)"] = _first_seen(battery, lambda i, img, rp: _fault_seam_compare(img, rp))
    print(f"\nC = {c}: first battery image that shows each wrong model")
    for k, (name, differs) in seen.items():
        print(f"  {k:50s} {name}  file differs: {differs}")
    assert all(name is not None and differs for name, differs in seen.values()), {k: v for k, v in seen.items() if not (v[0] and v[1])}


# ---------------------------------------------------------------------------------------------
# the float sources are exact
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("code", [0, 1, 2])
def test_float_sources_are_exact(code):
    """Every element of a float source is float_table(code, add)[byte]: the oracle quantiser gives the byte back for all 256
    entries of both tables, so for 100 % of the elements of every image -- none left out, none resampled."""
    for setname, (add, scale, bias) in W.FLOAT_SETS.items():
        tab = W.float_table(code, add)
        x = element_values(tab.view({0: np.float32, 1: np.float16, 2: np.uint16}[code]), code)
        assert np.array_equal(x, np.arange(256) + add), f"{setname}: the elements are not the integers they stand for"
        by = oracle_quantize(x, scale, bias)
        exact = float((by == np.arange(256)).mean())
        print(f"float code {code} set {setname}: {100 * exact:.0f} % of elements exact")
        assert exact == 1.0
        for c in (3, 4):   # ... and the long way, every element of every image
            for name, img in W.layout_battery(c):
                bits = W.float_bits(img, code, add)
                assert bits.shape == img.shape
                back = oracle_quantize(element_values(bits.view({0: np.float32, 1: np.float16, 2: np.uint16}[code]), code), scale, bias)
                assert np.array_equal(back, img), f"{setname} code {code}: {name}"
