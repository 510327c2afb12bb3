"""The optional check of a file's IDAT CRC-32 and Adler-32 on decode, on the drop-in's CPU tier (no GPU needed).

fpng::fpng_decode_memory reads FPNG_AMD_DECODE_VERIFY once per process, so every knob value gets a child process that decodes
the same list of files.  Python's zlib is the judge of every file (tests/verify_files.py): what a knob value must return follows
from zlib.crc32 over "IDAT" + payload and from zlib's own Adler check, not from the decoder.  The decoder's own answer is only
used for the unset case, which shows the premise: damage that keeps the stream in step decodes with status 0 today.

Files come from the reference build (oracle/_ref, through cpu_ref.ref()) where build() made it, else from the project's C
restatement of the encoder (cpu_ref.oracle()), which writes the same bytes."""
import hashlib
import json
import os
import pickle
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

from cpu_ref import have_ref, oracle, ref
import verify_files as vf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (5, 3), (257, 49), (300, 200)]
KNOBS = (None, 0, 1, 2, 3)

CHILD = r"""
import hashlib, json, os, pickle, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import dropin
cases = pickle.load(open(sys.argv[2], "rb"))
out = {}
for name, png, desired in cases:
    st, px, w, h, c = dropin.decode(png, desired)
    out[name] = [int(st), hashlib.sha1(px.tobytes()).hexdigest() if px is not None else None]
json.dump(out, open(sys.argv[3], "w"))
"""


def _writer():
    """which encoder writes the test's files: named in every assertion message"""
    return "reference build (oracle/_ref)" if have_ref() else "oracle() restatement: oracle/_ref is not built"


def _encode(img, w, h, c, flags):
    return (ref() if have_ref() else oracle()).encode(img, w, h, c, flags)


def _build_cases():
    import fpng_amd
    rng = np.random.default_rng(20261017)
    clean, damaged, failing = [], [], []  # (name, png, desired)
    for (w, h) in SIZES:
        for c in (3, 4):
            img = fpng_amd.synth_image("grad", w, h, c)
            for flags in (0, 1, 2):
                png = _encode(img, w, h, c, flags)
                assert png is not None
                name = f"{w}x{h}x{c}_f{flags}"
                assert not vf.crc_is_bad(png) and not vf.adler_is_bad(png), (name, _writer())  # what the encoders write is sound
                for desired in (3, 4):
                    clean.append((f"clean_{name}_d{desired}", png, desired))
                mode = vf.plan(png)[1]
                if mode == 0:
                    for where in (0.0, 0.5, 0.999):
                        good, stale, stale_crc = vf.edit_literal(png, where, rng)
                        tag = f"{name}_lit{where}"
                        damaged += [(f"good_{tag}", good, c), (f"stale_{tag}", stale, c), (f"stalecrc_{tag}", stale_crc, c)]
                        # one payload bit that the stream survives, the Adler-32 made right, the CRC not recomputed
                        o, l = vf.idat(good)
                        o0, l0 = vf.idat(png)
                        damaged.append((f"crconly_{tag}", good[:o + 8 + l] + png[o0 + 8 + l0:o0 + 12 + l0] + good[o + 12 + l:], c))
                else:
                    for (y, xb) in {(0, 0), (h // 2, (w * c) // 2), (h - 1, w * c - 1)}:
                        damaged.append((f"storedbyte_{name}_{y}_{xb}", vf.edit_stored_byte(png, w, h, c, y, xb), c))
                        damaged.append((f"storedbyte_nocrc_{name}_{y}_{xb}", vf.edit_stored_byte(png, w, h, c, y, xb, fix_crc=False), c))
                damaged.append((f"crcbit_{name}", vf.flip_crc_bit(png, int(rng.integers(0, 32))), c))
    # files that fail today: not an fpng file (the marker chunk's payload changed, its CRC made right), a bad IHDR CRC
    png = _encode(fpng_amd.synth_image("grad", 64, 32, 4), 64, 32, 4, 0)
    b = bytearray(png)
    i = png.index(b"fdEC")
    b[i + 4] ^= 1
    b[i + 9:i + 13] = struct.pack(">I", zlib.crc32(bytes(b[i:i + 9])))
    failing.append(("not_fpng", bytes(b), 4))
    b = bytearray(png)
    b[8 + 21] ^= 0x10
    failing.append(("ihdr_crc", bytes(b), 4))
    return clean, damaged, failing


# (the parameter only puts the files' writer into the ids of the tests that use them: a green run shows it too)
@pytest.fixture(scope="module", params=[None], ids=["files_by_reference_build" if have_ref() else "files_by_oracle_restatement"])
def answers(built_lib, tmp_path_factory):
    """{knob: {case name: (status, sha1 of the pixels)}} from one child process per knob value, and the cases"""
    clean, damaged, failing = _build_cases()
    d = tmp_path_factory.mktemp("verify_cpu")
    cases = d / "cases.pkl"
    pickle.dump(clean + damaged + failing, open(cases, "wb"))
    got = {}
    for knob in KNOBS:
        env = dict(os.environ)
        env.pop("FPNG_AMD_DECODE_VERIFY", None)
        env["FPNG_AMD_DECODE_CPU"] = "1"  # (every file here is far below the GPU tier's size anyway)
        if knob is not None:
            env["FPNG_AMD_DECODE_VERIFY"] = str(knob)
        out = d / f"out_{knob}.json"
        r = subprocess.run([sys.executable, "-c", CHILD, ROOT, str(cases), str(out)], env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        got[knob] = json.load(open(out))
    return got, clean, damaged, failing


def test_clean_files_decode_with_every_knob_value(answers):
    got, clean, _, _ = answers
    assert len(clean) == len(SIZES) * 2 * 3 * 2
    for name, png, desired in clean:
        st0, px0 = got[None][name]
        assert st0 == 0 and px0 is not None, (name, _writer())
        for knob in (0, 1, 2, 3):
            assert got[knob][name] == [0, px0], (name, _writer(), knob)


def test_premise_damage_that_keeps_the_stream_in_step_passes_by_default(answers):
    got, _, damaged, _ = answers
    kinds = set()
    for name, png, desired in damaged:
        assert got[None][name][0] == 0 and got[0][name][0] == 0, (name, _writer())
        kinds.add(name.split("_")[0])
    assert {"good", "stale", "stalecrc", "crconly", "storedbyte", "crcbit"} <= kinds


def test_damaged_files_get_what_zlib_says(answers):
    got, _, damaged, _ = answers
    seen = {65: 0, 66: 0, 0: 0}
    for name, png, desired in damaged:
        kind = name.split("_")[0]
        crc_bad, adler_bad = vf.crc_is_bad(png), vf.adler_is_bad(png)
        # the cases are what they claim to be (zlib's word): a one-byte change always moves s1 (|d| < 256 < 65521)
        want = {"good": (False, False), "stale": (False, True), "stalecrc": (True, True), "crconly": (True, False), "crcbit": (True, False)}.get(kind)
        if kind == "storedbyte":
            want = ("nocrc" in name, True)
        assert (crc_bad, adler_bad) == want, (name, _writer())
        for knob in (1, 2, 3):
            exp = vf.expected_status(png, knob)
            assert got[knob][name][0] == exp, (name, _writer(), knob, got[knob][name][0], exp)
            seen[exp] += 1
        if adler_bad:
            assert got[2][name][0] == 66 and got[3][name][0] == (65 if crc_bad else 66), (name, _writer())
        if crc_bad:
            assert got[1][name][0] == 65 and got[3][name][0] == 65, (name, _writer())
        if adler_bad and not crc_bad:
            assert got[1][name][0] == 0, (name, _writer())
        if kind == "good":  # a changed literal with both checksums right is simply another image
            assert [got[k][name][0] for k in (1, 2, 3)] == [0, 0, 0], (name, _writer())
    assert all(seen.values()), seen


def test_files_that_fail_today_keep_their_status(answers):
    got, _, _, failing = answers
    want = {"not_fpng": 1, "ihdr_crc": 4}  # fpng::FPNG_DECODE_NOT_FPNG, FPNG_DECODE_FAILED_HEADER_CRC32
    for name, png, desired in failing:
        for knob in KNOBS:
            assert got[knob][name][0] == want[name], (name, _writer(), knob)


def test_setter_rejects_unknown_bits(built_lib):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU: no encoder can be created")
    import fpng_amd
    enc = fpng_amd.Encoder(device=0)
    try:
        assert enc.decode_verify == 0
        assert enc.lib.fpng_amd_encoder_set_decode_verify(enc.h, 4) == -1  # FPNG_AMD_ERR_INVALID_ARG
        assert enc.lib.fpng_amd_encoder_set_decode_verify(enc.h, 7) == -1
        assert enc.decode_verify == 0  # nothing changed
        enc.set_decode_verify(fpng_amd.VERIFY_CRC32 | fpng_amd.VERIFY_ADLER32)
        assert enc.decode_verify == 3
        enc.set_decode_verify(0)
        assert enc.decode_verify == 0
    finally:
        enc.close()


def test_constants_and_symbols(built_lib):
    import fpng_amd
    from fpng_amd import _lib
    assert (fpng_amd.VERIFY_CRC32, fpng_amd.VERIFY_ADLER32, fpng_amd.DECODE_BAD_CRC32, fpng_amd.DECODE_BAD_ADLER32) == (1, 2, 65, 66)
    lib = _lib.load()
    assert lib.fpng_amd_encoder_set_decode_verify(None, 1) == -1 and lib.fpng_amd_encoder_decode_verify(None) == 0
    hdr = open(os.path.join(ROOT, "include", "fpng_amd.h")).read()
    for d in ("#define FPNG_AMD_VERIFY_CRC32 1u", "#define FPNG_AMD_VERIFY_ADLER32 2u", "#define FPNG_AMD_DECODE_BAD_CRC32 65", "#define FPNG_AMD_DECODE_BAD_ADLER32 66"):
        assert d in hdr
