"""The GPU decoder's STATUS on damaged and edited files, held to a deterministic judge (-m gpu).

* Small files (tests/test_decode_model.py: _damage, edited_files) in mixed batches: the status of every file must be the one the
  emulator of the kernels' own per-thread code gives at the kernels' constants (tests/cpp/decode_emul.cpp, CONFIGS[0]) --
  FPNG_AMD_DECODE_UNDECIDED only where the kernels' logic says so (a match at a row's first pixel, a record overflow, a stream
  that does not converge), never as a stand-in for NOT_FPNG.
* Tall files with ONE decidable token edit (tests/token_mutator.py: mutate_large with rows= and kind=) in the first, a middle or the
  last segment of rows, batched with clean tall files so that dec_unfilter_kernel's grid is several times what is resident: the
  edited file gets the reference's status, every other file its exact pixels, and no call stalls (a tile that skips its file
  without publishing its look-back granule makes the tiles of later segments spin to the limit)."""
import os
import struct
import time

import numpy as np
import pytest

import dropin
from cpu_ref import fuzz_image, have_ref, oracle, ref
from test_gpu_decode import UNDECIDED, _device_files, enc, judge  # noqa: F401  (enc: the module's fixture)

pytestmark = pytest.mark.gpu
GPU_MAX_ROUNDS = 64  # fpng_amd/csrc/decode_api.cpp: kMaxRounds (round 0 inside the workgroups, then up to 63 border rounds)


def _cpu_decode(png, desired):
    os.environ["FPNG_AMD_DECODE_CPU"] = "1"
    try:
        return dropin.decode(png, desired)
    finally:
        del os.environ["FPNG_AMD_DECODE_CPU"]


def _dims(pngs):
    out = []
    for p in pngs:
        w, h = struct.unpack(">II", bytes(p[16:24])) if len(p) >= 24 else (0, 0)
        out.append((w, h) if 0 < w <= (1 << 24) and 0 < h <= (1 << 24) and w * h <= (1 << 28) else (0, 0))
    return out


def _decode(enc, pngs, desired, device):
    if device:
        return enc.decode_device(_device_files(pngs, shift=1), desired, _dims(pngs))
    return enc.decode_batch(pngs, desired)


def _left_to_cpu_gives_the_judges_answer(png, desired, judged, what):
    cst, cpx, w, h, _ = judged
    dst, dpx, *_ = _cpu_decode(png, desired)
    assert dst == cst, (what, dst, cst)
    assert cst != 0 or np.array_equal(np.asarray(dpx)[: w * h * desired], np.asarray(cpx)[: w * h * desired]), what


# ---- a. small files: the GPU's status is the kernels' logic ----
def _small_files(rng):
    """[(name, file)]: valid files, the same files damaged (bit flips, truncations, header and stream bytes), token-edited files"""
    from test_decode_model import _damage, edited_files
    valid, bad = [], []
    for _ in range(40):
        img, w, h, c = fuzz_image(rng) if rng.random() < 0.6 else fuzz_image(rng, force_dims=(int(rng.integers(100, 400)), int(rng.integers(4, 40))))
        png = oracle().encode(img, w, h, c, int(rng.integers(0, 2)))
        valid.append(("valid", png))
        for _ in range(4):
            kind, d = _damage(rng, png)
            bad.append((f"damage{kind}", d))
    bad += edited_files(rng, 30)
    return valid, bad


def _batches(rng, valid, bad):
    """batches of 8..30 files: damaged / edited ones in order, 2..6 valid ones mixed in at random places"""
    out, k = [], 0
    while k < len(bad):
        n_valid = int(rng.integers(2, 7))
        n_bad = min(len(bad) - k, int(rng.integers(8, 31)) - n_valid)
        b = bad[k:k + n_bad]
        k += n_bad
        for _ in range(n_valid):
            b.insert(int(rng.integers(0, len(b) + 1)), valid[int(rng.integers(0, len(valid)))])
        out.append(b)
    return out


@pytest.mark.parametrize("desired", [3, 4])
def test_status_is_the_kernels_logic_on_small_damaged_files(enc, desired):
    """Every file's status from both batch entry points equals the emulator's at CONFIGS[0] with the GPU's round limit; pixels of the
    judge where that is 0; where it is UNDECIDED, the drop-in's CPU decoder gives the judge's answer."""
    from test_decode_model import CONFIGS, emul_decode
    rng = np.random.default_rng(606 + desired)
    valid, bad = _small_files(rng)
    batches = _batches(rng, valid, bad)
    model, judged = {}, {}
    near_limit = most_rounds = 0
    for b in batches:
        for name, f in b:
            if f in model:
                continue
            st, _, _, _, _, stats = emul_decode(f, desired, CONFIGS[0], border_rounds=GPU_MAX_ROUNDS - 1)
            model[f] = st
            judged[f] = judge(f, desired) if len(f) else (2, None, 0, 0, 0)
            most_rounds = max(most_rounds, stats[1])
            near_limit += stats[1] >= GPU_MAX_ROUNDS // 2
    # (no file comes near the round limit: there the GPU's rounds, launched in fours, and the emulator's could part)
    assert near_limit == 0, (near_limit, most_rounds)
    counts = {}
    for device in (False, True):
        for b in batches:
            got = _decode(enc, [f for _, f in b], desired, device)
            for i, ((name, f), (st, px, cf)) in enumerate(zip(b, got)):
                what = (name, device, i, len(b))
                assert st == model[f], (what, st, model[f])
                cst, cpx, w, h, c = judged[f]
                if st == UNDECIDED:
                    _left_to_cpu_gives_the_judges_answer(f, desired, judged[f], what)
                else:
                    assert st == cst, (what, st, cst)
                if st == 0:
                    assert cf == c and np.array_equal(px.cpu().numpy().reshape(-1), np.asarray(cpx)[: w * h * desired]), what
                counts[st] = counts.get(st, 0) + 1
    # (the mix: files that decode, that are rejected, and a few left to the CPU decoder by the kernels' logic)
    assert counts.get(0, 0) >= 200 and sum(v for k, v in counts.items() if k not in (0, UNDECIDED)) >= 200 and counts.get(UNDECIDED, 0) >= 4, counts


# ---- b. one decidable edit deep in a tall file, in batches bigger than the resident grid ----
TALL = {  # name: (synth kind, w, h, c, flags)
    "4k_rgba": ("grad", 3840, 2160, 4, 0),         # 45 segments x 15 column blocks, IDAT over 8 MiB (decode_host streams it)
    "tall_rgb_2pass": ("glyphs", 1024, 4320, 3, 1),  # 90 segments x 4 (tests/ui_images.py: text and flat areas, many matches)
    "blocks_rgb": ("blocks", 2048, 1500, 3, 0),    # 32 segments x 8
}
# decided inside dec_unfilter_kernel's walk (NOT_FPNG), a filter literal (kDecBadFilter: the control), and a match at a row's
# first pixel (the reference takes it; the kernels leave it to the CPU decoder by design)
EDITS = ("match_over_row_end", "match_plus_a_byte", "match_minus_a_byte", "filter_byte", "lit2match_firstpx")
ROWS = 48  # fpng_amd/csrc/decode.h: kDecUnfRows


def _encode(img, w, h, c, flags):
    # (the reference's encoder; where its build is absent, the C restatement, which writes the same bytes: tests/test_oracle.py)
    return (ref() if have_ref() else oracle()).encode(img, w, h, c, flags)


def _placements(h):
    nseg = (h + ROWS - 1) // ROWS
    return {"first": (0, ROWS - 1), "quarter": (h // 4, h // 4 + ROWS - 1), "half": (h // 2, h // 2 + ROWS - 1), "last": ((nseg - 1) * ROWS, h - 1)}


def _edited(s, rng, kind, rows):
    """a file with one edit of this kind in these rows that the judge rejects (lit2match_firstpx: any); None if none was found (the
    match edits need a length that the file's Huffman table codes: a gradient's table has few)"""
    import token_mutator as TM
    for _ in range(150):
        name, f = TM.mutate_large(s, rng, rows=rows, kind=kind)
        if f is None:
            continue
        assert name == kind
        judged = {d: judge(f, d) for d in (3, 4)}
        if kind == "lit2match_firstpx" or judged[3][0] != 0:
            return f, judged
    return None


def _want(t, desired):
    import torch
    c = t.shape[2]
    return t[:, :, :desired] if c >= desired else torch.cat([t, torch.full_like(t[:, :, :1], 255)], dim=2)


def test_decidable_edits_deep_in_tall_batches(enc):
    """Every edit of EDITS at every placement of _placements in every base of TALL, inside a batch of four tall files (all of the
    same base, or of mixed heights so that the pieces of segments change), at every position of the batch, through both batch entry
    points: the edited file has the judge's status (UNDECIDED only for lit2match_firstpx, and then the drop-in's CPU decoder gives
    the judge's answer), every other file its exact pixels, and no call takes more than 3 x the clean batch's time + 0.15 s.  The
    edited 4K RGBA files also go through fpng_amd_decode_host, which streams them, under the same rules."""
    import torch
    import fpng_amd
    import test_decode_model as M
    import token_mutator as TM
    import ui_images
    rng = np.random.default_rng(2160)
    base, want, edits = {}, {}, []
    for bi, (name, (kind, w, h, c, flags)) in enumerate(TALL.items()):
        img = ui_images.glyphs(w, h, c, seed=5) if kind == "glyphs" else fpng_amd.synth_image(kind, w, h, c)
        base[name] = _encode(np.ascontiguousarray(img).reshape(-1), w, h, c, flags)
        t = torch.from_numpy(img).cuda()
        want[name] = {d: _want(t, d) for d in (3, 4)}
        s = TM.LargeStream(base[name], M.plan, M.emul())
        for kind in EDITS:
            for where, rows in _placements(h).items():
                got = _edited(s, rng, kind, rows)
                assert got is not None or kind.startswith("match"), (name, kind, where)
                if got is not None:
                    edits.append((name, kind, where, got[0], got[1]))
        del s
    # every edit at every placement in some base, and every base with edits at all four placements
    assert {(k, p) for _, k, p, _, _ in edits} == {(k, p) for k in EDITS for p in ("first", "quarter", "half", "last")}
    assert len(edits) >= 50, len(edits)
    assert len(base["4k_rgba"]) > (8 << 20) + 100  # (decode_host streams it)
    names = list(TALL)
    clean_time = {}

    def timed(files, desired, device):
        if device:
            dev = _device_files(files, shift=1)
            dims = _dims(files)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = enc.decode_device(dev, desired, dims)
        else:
            t0 = time.perf_counter()
            got = enc.decode_batch(files, desired)
        return got, time.perf_counter() - t0

    def t_clean(layout, desired, device):
        key = (layout, desired, device)
        if key not in clean_time:
            files = [base[n] for n in layout]
            timed(files, desired, device)  # (warm-up)
            runs = []
            for _ in range(2):
                got, dt = timed(files, desired, device)
                assert all(st == 0 for st, _, _ in got), key
                runs.append(dt)
            clean_time[key] = min(runs)
        return clean_time[key]

    slowest = (0.0, None)
    for k, (name, kind, where, f, judged) in enumerate(edits):
        desired = 3 + (k // 2) % 2
        pos = k % 4
        if k % 3 == 2:  # mixed heights: the edited file's base at `pos` and one more, the two other bases between
            others = [n for n in names if n != name]
            layout = tuple(np.roll(np.array([name, others[0], others[1], name], dtype=object), pos))
        else:
            layout = (name,) * 4
        assert layout[pos] == name
        files = [base[n] for n in layout]
        files[pos] = f
        cst, cpx, w, h, c = judged[desired]
        for device in (False, True):
            t0 = t_clean(layout, desired, device)
            got, dt = timed(files, desired, device)
            what = (name, kind, where, layout, pos, desired, device)
            assert dt <= 3 * t0 + 0.15, (what, dt, t0)
            if dt > slowest[0]:
                slowest = (dt, what, t0)
            for i, (st, px, cf) in enumerate(got):
                if i != pos:
                    assert st == 0 and torch.equal(px, want[layout[i]][desired]), (what, i, st)
                    continue
                if st == UNDECIDED:
                    assert kind == "lit2match_firstpx", (what, st, cst)
                    _left_to_cpu_gives_the_judges_answer(f, desired, judged[desired], what)
                    continue
                assert st == cst, (what, st, cst)
                if st == 0:
                    assert np.array_equal(px.cpu().numpy().reshape(-1), np.asarray(cpx)[: w * h * desired]), what
    print(f"\nslowest damaged batch call {slowest[0] * 1e3:.1f} ms {slowest[1]}, its clean batch {slowest[2] * 1e3:.1f} ms; "
          f"clean batches {min(clean_time.values()) * 1e3:.1f} .. {max(clean_time.values()) * 1e3:.1f} ms")

    # the streamed host path (fpng_amd_decode_host: the 4K RGBA file's IDAT is over 8 MiB)
    host_clean = {}
    slowest_host = 0.0
    for k, (name, kind, where, f, judged) in enumerate(e for e in edits if e[0] == "4k_rgba"):
        desired = 3 + k % 2
        if desired not in host_clean:
            enc.decode_host(base[name], desired)  # (warm-up)
            runs = []
            for _ in range(2):
                t0 = time.perf_counter()
                st, px, _ = enc.decode_host(base[name], desired)
                runs.append(time.perf_counter() - t0)
                assert st == 0 and np.array_equal(px, want[name][desired].cpu().numpy())
            host_clean[desired] = min(runs)
        t0 = time.perf_counter()
        st, px, cf = enc.decode_host(f, desired)
        dt = time.perf_counter() - t0
        what = (name, kind, where, desired, "host")
        assert dt <= 3 * host_clean[desired] + 0.15, (what, dt, host_clean[desired])
        slowest_host = max(slowest_host, dt)
        cst, cpx, w, h, c = judged[desired]
        if st == UNDECIDED:
            assert kind == "lit2match_firstpx", (what, st, cst)
            _left_to_cpu_gives_the_judges_answer(f, desired, judged[desired], what)
            continue
        assert st == cst, (what, st, cst)
        if st == 0:
            assert np.array_equal(px.reshape(-1), np.asarray(cpx)[: w * h * desired]), what
    print(f"decode_host: clean {min(host_clean.values()) * 1e3:.1f} ms, slowest damaged {slowest_host * 1e3:.1f} ms")
