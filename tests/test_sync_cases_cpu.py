"""The streams of tests/sync_cases.py, held to their names on the CPU: every case is a valid file (the reference's decoder, or its
recorded answers, judges), the kernels' per-thread code run with the kernels' constants (tests/cpp/decode_emul.cpp) decodes it to
the judge's pixels, and the emulator's TRACE shows the property the case was built for -- which branch of dec_sync_kernel its
blocks take, where its stream ends, how many walks its windows have.  A case that no longer has its property (a constant of the
kernels changed, an encoder's output changed) fails here and is named; tests/test_gpu_decode_sync_geometry.py then runs the same
files on the GPU."""
import numpy as np
import pytest

import sync_cases as S
from cpu_ref import ref
from test_decode_model import CONFIGS, emul_decode

NAMES = {g: [c.name for c in cs] for g, cs in (("A", S.group_a()), ("B", S.group_b()), ("D", S.group_d()))}  # (names only: nothing is built yet)
BATCHES = ["C.batch.1", "C.batch.63", "C.batch.64", "C.batch.65", "C.batch.64.no_stored", "C.batch.65.no_stored", "C.files.64.with_stored"]


@pytest.fixture(scope="module")
def cases():
    c = S.all_cases()
    assert [b.name for b in c["C"]] == BATCHES
    return {x.name: x for g in c.values() for x in g}


def _judged(png, name):
    """the file is valid and the kernels' logic decodes it to the judge's pixels, to 3 and to 4 channels"""
    for desired in (3, 4):
        st_r, out_r, w, h, c = ref().decode(png, desired)
        assert st_r == 0, (name, desired, st_r)
        st, px, ww, hh, cc, _ = emul_decode(png, desired, CONFIGS[0])
        assert st == 0 and (ww, hh, cc) == (w, h, c), (name, desired, st)
        assert np.array_equal(px, np.asarray(out_r)[: px.size]), (name, desired)


@pytest.mark.parametrize("name", NAMES["A"] + NAMES["B"] + NAMES["D"])
def test_case_is_valid_and_shows_its_property(cases, name):
    case = cases[name]
    assert len(case.png) <= 80 * 1024 and case.trace.n_sub <= 1100 and case.trace.h <= 400 and case.trace.c in (3, 4), name
    _judged(case.png, name)
    assert not case.missing(), f"{name} no longer has the property it was built for: {case.missing()}"


@pytest.mark.parametrize("name", BATCHES)
def test_batch_is_valid_and_shows_its_property(cases, name):
    batch = cases[name]
    for k, f in enumerate(batch.files):
        if batch.modes[k]:  # (a stored file: no subsequences, nothing for the kernels' logic to settle)
            assert ref().decode(f, 4)[0] == 0, (name, k)
        else:
            _judged(f, (name, k))
    assert not batch.holds(), f"{name} no longer has the properties it was built for: {batch.holds()}"


def test_every_property_is_hit(cases):
    """The full list of tests/sync_cases.py (groups A to D) -- but for the properties that cannot be had, whose argument
    test_what_cannot_be_had_stays_out_of_reach holds to the traces."""
    hit = set()
    for x in cases.values():
        missing = x.holds() if x.group == "C" else x.missing()
        hit |= set(x.props) - set(missing)
    assert hit == set(S.ALL_PROPS) - set(S.UNREACHABLE), (sorted(set(S.ALL_PROPS) - set(S.UNREACHABLE) - hit), sorted(hit - set(S.ALL_PROPS)))


def test_what_cannot_be_had_stays_out_of_reach(cases):
    """sync_cases.UNREACHABLE: a block that round 0 settled has, in a border round, ONE thread to correct per step until its phase
    maps are used -- in every trace of every case.  (Were it otherwise, kGatherMin and more could be had there, and a case is due.)"""
    opened = 0
    for x in cases.values():
        for tr in ([x.trace] if x.group != "C" else []):
            for b in tr.blocks:
                if b["round"] >= 1 and tr.block(b["blk"], 0)["left"] == 0:
                    opened += 1
                    for s in tr.steps:
                        if s["round"] == b["round"] and s["blk"] == b["blk"] and s["kind"] == S.KIND_REDO and not b["maps"]:
                            assert s["n_need"] == 1, (x.name, b, s["it"], s["n_need"])
    assert opened >= 1


def test_derived_bounds_of_the_walks():
    """Group D's bounds (sync_cases.py has the derivation): 42 bytes at least from a subsequence that is neither first nor last,
    26 walks at most for a window of 256 four-byte pixels, 20 for three-byte ones -- under dec_unfilter_kernel's kMaxWalksPerRow."""
    assert (S.MIN_SUB_BYTES, S.max_walks(4), S.max_walks(3)) == (42, 26, 20)
    assert max(S.max_walks(3), S.max_walks(4)) <= S.MAX_WALKS_PER_ROW
    import os
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fpng_amd", "csrc", "decode.hip")).read()
    assert f"constexpr uint32_t kMaxWalksPerRow = {S.MAX_WALKS_PER_ROW};" in src and f"constexpr uint32_t kGatherMin = {S.GATHER_MIN};" in src


@pytest.mark.parametrize("name, bits", [("A.end.straddles.block.1pass", 12), ("A.n_sub.513.padding", 1), ("B.need0.64", None)])
def test_a_case_that_loses_its_property_is_caught(cases, name, bits):
    """The stream's end moved on by a literal's worth of bits (the code no longer straddles the border; no longer ends on it), a
    block's content changed: the predicate that passes for the case fails for the changed file."""
    case = next(c for c in cases.values() if name in c.props)
    assert S.PROPS[name](case.trace)
    if bits is None:  # the file of another count
        other = S.Trace(cases["B.need0.65"].png)
    else:
        changed = S.retimed(case.png, bits)
        assert changed is not None
        other = S.Trace(changed)
    assert other.status == 0 and not S.PROPS[name](other), name

