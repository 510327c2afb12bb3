"""CPU tests of the decoder half of the `namespace fpng` drop-in (fpng_amd/csrc/fpng_decode.cpp)
against the reference decoder: same pixels, same status codes, including on damaged files."""
import os

import numpy as np
import pytest

import dropin
from cpu_ref import fuzz_image, have_ref, have_ref_answers, oracle, ref


def test_roundtrip_all_channel_conversions():
    rng = np.random.default_rng(31)
    for _ in range(150):
        img, w, h, c = fuzz_image(rng)
        for fl in (0, 1, 2):
            png = oracle().encode(img, w, h, c, fl)
            assert dropin.get_info(png) == (0, w, h, c)
            for desired in (3, 4):
                st, out, ww, hh, cc = dropin.decode(png, desired)
                assert st == 0 and (ww, hh, cc) == (w, h, c)
                exp = img.reshape(h, w, c)
                if desired == c:
                    exp2 = exp
                elif desired == 3:
                    exp2 = exp[:, :, :3]
                else:
                    exp2 = np.concatenate([exp, np.full((h, w, 1), 255, dtype=np.uint8)], axis=2)
                assert (out == exp2.reshape(-1)).all(), (w, h, c, fl, desired)


@pytest.mark.skipif(not have_ref_answers(), reason="neither the reference build nor its recorded answers")
def test_status_codes_match_reference_on_damaged_files():
    rng = np.random.default_rng(32)
    checked = differing = 0
    for _ in range(120):
        img, w, h, c = fuzz_image(rng)
        png = bytearray(oracle().encode(img, w, h, c, int(rng.integers(0, 3))))
        for _ in range(12):
            bad = bytearray(png)
            kind = rng.integers(0, 4)
            if kind == 0:      # flip a bit anywhere
                i = int(rng.integers(0, len(bad)))
                bad[i] ^= 1 << int(rng.integers(0, 8))
            elif kind == 1:    # truncate
                bad = bad[: int(rng.integers(0, len(bad)))]
            elif kind == 2:    # damage the header region
                i = int(rng.integers(0, min(58, len(bad))))
                bad[i] = int(rng.integers(0, 256))
            else:              # damage the zlib stream
                i = int(rng.integers(58, len(bad)))
                bad[i] = int(rng.integers(0, 256))
            bad = bytes(bad)
            if not bad:
                continue
            for desired in (3, 4):
                st_r, out_r, *_ = ref().decode(bad, desired)
                st_m, out_m, *_ = dropin.decode(bad, desired)
                checked += 1
                assert st_r == st_m, (w, h, c, kind, st_r, st_m)
                if st_r == 0:
                    assert (out_r == out_m).all()
    assert checked > 2000


def test_large_image_decodes_with_or_without_a_gpu():
    """Images of 256K pixels and more take the drop-in's GPU tier when the process has a GPU (tests/test_gpu_decode.py holds that
    one against the reference decoder); without one -- this container -- the same call must quietly use the CPU decoder."""
    import fpng_amd
    img = fpng_amd.synth_image("grad", 1024, 768, 3)
    for fl in (0, 1, 2):
        png = oracle().encode(img, 1024, 768, 3, fl)
        for desired in (3, 4):
            st, out, w, h, c = dropin.decode(png, desired)
            assert st == 0 and (w, h, c) == (1024, 768, 3)
            exp = img if desired == 3 else np.concatenate([img, np.full((768, 1024, 1), 255, dtype=np.uint8)], axis=2)
            assert np.array_equal(out, exp.reshape(-1))


def test_not_png_and_bad_args():
    assert dropin.get_info(b"hello world, definitely not a png file at all, padding padding padding padding")[0] == 3  # FAILED_NOT_PNG
    png = oracle().encode(np.zeros((4, 4, 3), dtype=np.uint8), 4, 4, 3, 0)
    st, *_ = dropin.decode(png, 5)
    assert st == 2  # FPNG_DECODE_INVALID_ARG (reference fpng.cpp:3092-3096)


def test_checksum_wrappers():
    import zlib
    d = np.random.default_rng(1).integers(0, 256, 4097, dtype=np.uint8)
    L = dropin.shim()
    assert L.shim_crc32(d.ctypes.data, d.size, 0) == zlib.crc32(d.tobytes())
    assert L.shim_adler32(d.ctypes.data, d.size, 1) == zlib.adler32(d.tobytes())


def edited_containers(rng, n_images, per_image=10):
    """[(name of the edit, file)]: chunk-level and block-level edits with the CRCs made good again (tests/container_mutator.py)"""
    import container_mutator as CM
    out = []
    for _ in range(n_images):
        img, w, h, c = fuzz_image(rng)
        png = oracle().encode(img, w, h, c, int(rng.integers(0, 3)))
        for _ in range(per_image):
            name, f = CM.mutate(png, rng)
            if name != "none":
                out.append((name, f))
    return out


@pytest.mark.skipif(not have_ref_answers(), reason="the reference's decoder (or its recorded answers) is the judge")
def test_container_and_block_edits_get_the_references_answer():
    """A flipped bit in a PNG container ends at the chunk's CRC.  These files carry good CRCs and odd STRUCTURE: chunks inserted,
    missing, doubled or out of order, IHDR fields and dimensions changed, several IDATs, junk behind IEND, other zlib headers and
    block types, stored blocks cut into other sizes or with damaged headers (incl. the one zero byte behind the image that the
    reference lets pass: src/fpng.cpp:2158-2166), dynamic headers with other counts.  fpng_get_info and fpng_decode_memory of the
    reference judge; the drop-in's functions and the GPU decoder's host side (fpng_amd_decode_plan + the kernels' logic on the
    CPU; UNDECIDED = the drop-in's CPU decoder answers) must agree in status, geometry and pixels."""
    import test_decode_model as M
    rng = np.random.default_rng(606)
    R = ref()
    seen, accepted, left = set(), 0, 0
    for name, f in edited_containers(rng, 260):
        gst, *whc = R.get_info(f)
        mine = dropin.get_info(f)
        assert mine[0] == gst and (gst != 0 or mine[1:] == tuple(whc)), (name, gst, mine)
        desired = int(rng.choice([3, 4]))
        st_r, out_r, *dr = R.decode(f, desired)
        st_c, out_c, *dc = dropin.decode(f, desired)
        st_m, out_m, *_ = M.emul_decode(f, desired, M.CONFIGS[int(rng.integers(0, len(M.CONFIGS)))])
        if st_m == M.UNDECIDED:
            left += 1
            st_m, out_m = st_c, out_c
        assert st_c == st_r and st_m == st_r, (name, st_r, st_c, st_m)
        if st_r == 0:
            accepted += 1
            assert dr == dc and np.array_equal(out_r, out_c) and np.array_equal(np.asarray(out_r)[: out_m.size], out_m), name
        seen.add(name)
    assert len(seen) >= 30 and accepted >= 150 and left >= 20, (len(seen), accepted, left)
    # the reference's quirk, on purpose: ONE zero byte behind a stored image passes, anything else behind it does not
    import container_mutator as CM
    for (w, h, c) in ((3, 2, 3), (5, 4, 4), (300, 250, 3)):  # (the last one: more than one 65535-byte block)
        img = rng.integers(0, 256, w * h * c, dtype=np.uint8)
        png = oracle().encode(img, w, h, c, 2)
        for tail, want in ((b"", 0), (b"\0", 0), (b"\1", 1), (b"\0\0", 1), (b"\0\5", 1)):
            f = CM.stored_with_tail(png, tail)
            for desired in (3, 4):
                st_r, out_r, *_ = R.decode(f, desired)
                st_c, out_c, *_ = dropin.decode(f, desired)
                st_m, out_m, *_ = M.emul_decode(f, desired)
                assert st_r == want and st_c == want, (w, h, c, tail, st_r, st_c)
                assert st_m == (M.UNDECIDED if tail == b"\0" else want), (w, h, c, tail, st_m)  # (the odd layout is the CPU decoder's)
                if want == 0:
                    assert np.array_equal(out_r, out_c) and np.array_equal(out_c, M.expected_pixels(img, w, h, c, desired))


def other_tables(rng, n_images, per_image=8):
    """[(what was done, file)]: token streams (as they are, edited, or with the reserved length symbols 286 / 287 put in) written
    again under random dynamic Huffman tables (tests/header_mutator.py)"""
    import header_mutator as HM
    import test_decode_model as M
    import token_mutator as TM
    out = []
    for _ in range(n_images):
        img, w, h, c = fuzz_image(rng) if rng.random() < 0.6 else fuzz_image(rng, force_dims=(int(rng.integers(20, 300)), int(rng.integers(2, 12))))
        png = oracle().encode(img, w, h, c, int(rng.integers(0, 2)))
        if M.plan(png)[1]:
            continue
        s = TM.Stream(png, M.plan)
        for k in range(per_image):
            toks, tag = None, ""
            if k >= 5:
                toks, tag = HM.with_reserved_symbols(s, rng), "+sym"
            elif k >= 3:
                toks, _ = TM.mutate(s, rng)
                if rng.random() < 0.5:
                    toks = TM.balanced(s, toks, rng)
            name, f = HM.reencode(s, rng, toks)
            out.append((name + tag, c, f))
    return out


@pytest.mark.skipif(not have_ref_answers(), reason="the reference's decoder (or its recorded answers) is the judge")
def test_other_huffman_tables_and_the_reserved_length_symbols():
    """The block header's reader and the table builders under tables no fpng encoder writes: random complete codes up to 12 bits
    (and longer: turned away), single-code tables, HLIT / HDIST / HCLEN larger than needed, the code lengths spelled with the repeat
    symbols in every way, distance tables the reference lets through (one or two 1-bit codes, other lengths next to them) or not.
    And the length symbols 286 / 287: the reference's 4-channel decoder takes them for matches of length zero whose copy loop runs
    once (src/fpng.cpp:2668-2760) -- the drop-in's CPU decoder does the same, the GPU decoder's host side leaves such tables to it.
    Status and pixels of the reference."""
    import test_decode_model as M
    rng = np.random.default_rng(909)
    R = ref()
    accepted = reserved_accepted = left = 0
    seen = set()
    for name, c, f in other_tables(rng, 45):
        desired = int(rng.choice([3, 4]))
        st_r, out_r, *_ = R.decode(f, desired)
        st_c, out_c, *_ = dropin.decode(f, desired)
        st_m, out_m, *_ = M.emul_decode(f, desired, M.CONFIGS[int(rng.integers(0, len(M.CONFIGS)))])
        if st_m == M.UNDECIDED:
            left += 1
            st_m, out_m = st_c, out_c
        assert st_c == st_r and st_m == st_r, (name, c, st_r, st_c, st_m)
        if st_r == 0:
            accepted += 1
            reserved_accepted += name.endswith("+sym")
            assert np.array_equal(out_r, out_c) and np.array_equal(np.asarray(out_r)[: out_m.size], out_m), name
        seen |= set(name.split("+"))
    assert accepted >= 70 and reserved_accepted >= 5 and left >= 20, (accepted, reserved_accepted, left)
    assert {"codes_longer_than_12", "kraft_off", "all_symbols", "two_dist_codes", "other_dist_lengths", "reserved_symbols_coded"} <= seen, seen


def test_cpu_decoder_under_the_sanitizers(tmp_path):
    """fpng_decode.cpp built with AddressSanitizer + UndefinedBehaviorSanitizer over a few thousand valid, damaged and hand-edited files
    (containers, stored blocks, tokens, other Huffman tables, reserved symbols), each decoded from an exact-size copy: its row
    buffers are written with 4- to 16-byte stores that run past the bytes wanted -- the slack must always be there."""
    import shutil
    import subprocess
    import test_decode_model as M
    from cpu_ref import ROOT
    if not shutil.which("g++"):
        pytest.skip("no g++")
    rng = np.random.default_rng(5150)
    files = [f for _, f in edited_containers(rng, 60)] + [f for _, _, f in other_tables(rng, 25)] + [f for _, f in M.edited_files(rng, 25)]
    for _ in range(150):
        img, w, h, c = fuzz_image(rng)
        png = oracle().encode(img, w, h, c, int(rng.integers(0, 3)))
        files.append(png)
        for _ in range(4):
            bad = bytearray(png)
            if rng.random() < 0.3:
                bad = bad[: int(rng.integers(1, len(bad)))]
            else:
                bad[int(rng.integers(0, len(bad)))] ^= 1 << int(rng.integers(0, 8))
            files.append(bytes(bad))
    corpus = tmp_path / "corpus.bin"
    with open(corpus, "wb") as f:
        for p in files:
            f.write(len(p).to_bytes(4, "little") + p)
    exe = str(tmp_path / "drv")
    csrc = os.path.join(ROOT, "fpng_amd", "csrc")
    lib_dir = os.path.join(ROOT, "fpng_amd", "lib")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "include"), "-I", csrc,
                        os.path.join(ROOT, "tests", "cpp", "decoder_sanitizer_driver.cpp"), os.path.join(csrc, "fpng_decode.cpp"), os.path.join(csrc, "fpng_dropin.cpp"),
                        "-o", exe, "-L", lib_dir, "-lfpng_amd", "-Wl,-rpath," + lib_dir], capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr:
        pytest.skip("this g++ has no sanitizer runtime")
    assert r.returncode == 0, r.stderr[-800:]
    env = dict({k: v for k, v in os.environ.items() if k != "LD_PRELOAD"}, FPNG_AMD_DECODE_CPU="1", ASAN_OPTIONS="detect_leaks=0")
    q = subprocess.run([exe, str(corpus)], capture_output=True, text=True, env=env, timeout=600)
    assert q.returncode == 0 and "Sanitizer" not in q.stderr and "runtime error" not in q.stderr, q.stderr[-1500:]
    n, ok = int(q.stdout.split()[0]), int(q.stdout.split()[2])
    assert n == 2 * len(files) and 0.2 * n < ok < 0.9 * n, q.stdout


@pytest.mark.skipif(not have_ref_answers(), reason="the reference's decoder (or its recorded answers) is the judge")
def test_flat_rows_with_a_run_at_the_first_pixel():
    """The CPU decoder copies the row above where a row is its first pixel of zero literals + runs of zero deltas.  Hand-made rows
    that LOOK like that by their byte counts: a run of zeros that starts at the first pixel (the reference takes it: the pixel in
    front of a row is zeros) followed by literal pixels that are not zero -- the short cut must not fire."""
    import test_decode_model as M
    import token_mutator as TM
    for c in (3, 4):
        w, h = 30, 6
        img = np.full((h, w, c), 90, dtype=np.uint8)  # flat: every row after the first is [2][zero pixel][runs of zeros]
        s = TM.Stream(oracle().encode(img.reshape(-1), w, h, c, 0), M.plan)  # (1-pass: the trained table has a code for every symbol)
        pos = s.positions()
        rows = [i for i, t in enumerate(s.tokens) if t[0] == "lit" and pos[i] % s.stride == 0]
        T = list(s.tokens)
        i = rows[3]  # the fourth row: filter literal, c zero literals, matches
        assert all(T[i + 1 + k] == ("lit", 0) for k in range(c)) and T[i + 1 + c][0] == "match"
        run = T[i + 1 + c][1]
        # the first pixel's literals + the first run -> ONE run from the first pixel on, a pixel shorter; a literal pixel of 7s makes up for it
        T[i + 1:i + 2 + c] = [("match", run, 0)] + [("lit", 7)] * c
        f = s.write(T)
        assert f is not None
        for desired in (3, 4):
            st_r, out_r, *_ = ref().decode(f, desired)
            st_c, out_c, *_ = dropin.decode(f, desired)
            assert st_r == 0 and st_c == 0 and np.array_equal(out_r, out_c)
            px = np.asarray(out_c).reshape(h, w, desired)
            assert (px[3, run // c, :3] == 97).all() and (px[2, :, :3] == 90).all()  # (the literal pixel's deltas arrived)


def _vector_size_fn(lib, name):
    import ctypes as C
    f = getattr(lib, name)
    f.restype = C.c_size_t
    f.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_size_t, C.POINTER(C.c_int)]

    def call(png, desired, prefill):
        b = np.frombuffer(bytes(png), dtype=np.uint8)
        st = C.c_int(0)
        n = f(b.ctypes.data if b.size else None, b.size, desired, prefill, C.byref(st))
        return st.value, n
    return call


@pytest.mark.skipif(not have_ref(), reason="the reference's decoder is the judge")
def test_vector_size_on_every_exit():
    """fpng_decode_memory empties `out` on entry and sizes it once the container is accepted (src/fpng.cpp:3087-3111): a caller who
    reuses one vector sees size 0 after a container-level failure and width*height*desired after a failure inside the stream.
    Same sizes out of the drop-in on every exit: bad arguments, every container status, stream failures, success."""
    import container_mutator as CM
    mine = _vector_size_fn(dropin.shim(), "shim_decode_vector_size")
    theirs = _vector_size_fn(ref().L, "ref_decode_vector_size")
    rng = np.random.default_rng(909)
    files = [b"", b"x", b"\x89PNG\r\n\x1a\n" + bytes(60)]
    for _ in range(60):
        img, w, h, c = fuzz_image(rng)
        png = oracle().encode(img, w, h, c, int(rng.integers(0, 3)))
        files.append(png)
        files.append(png[: int(rng.integers(1, len(png)))])
        for _ in range(4):
            bad = bytearray(png)
            bad[int(rng.integers(58, len(bad) - 16))] ^= 1 << int(rng.integers(0, 8))  # the stream: no CRC guards it
            files.append(bytes(bad))
        for _ in range(6):
            files.append(CM.mutate(png, rng)[1])
    seen = {}
    for f in files:
        for desired in (3, 4, 5):
            if not f and desired != 5:
                continue
            for prefill in (0, 1000):
                a, b = theirs(f, desired, prefill), mine(f, desired, prefill)
                assert a == b, (len(f), desired, prefill, a, b)
                seen[(a[0], a[1] > 0)] = seen.get((a[0], a[1] > 0), 0) + 1
    # success, stream failure with a sized vector, container failures with an empty one
    assert seen.get((0, True), 0) > 50 and seen.get((1, True), 0) > 50 and sum(v for (st, sized), v in seen.items() if st > 1 and not sized) > 50, seen
    assert not any(sized for (st, sized) in seen if st > 1), seen


@pytest.mark.skipif(not have_ref() or not os.path.exists(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref", "libfpng_ref_nocrc.so")),
                    reason="the reference built with FPNG_DISABLE_DECODE_CRC32_CHECKS=1 is the judge")
def test_disable_decode_crc32_checks_build():
    """FPNG_DISABLE_DECODE_CRC32_CHECKS (src/fpng.cpp:10, :50-53, :3016-3023): the reference's compile-time switch for fuzzing
    skips the CRC-32 of every chunk behind IHDR (IHDR's own is still checked, :2960).  fpng_amd/csrc/png_parse.h carries the
    same switch; the drop-in's decoder built with it against the reference built with it, on files whose chunk CRCs are wrong:
    same status, same geometry, same pixels -- and the default builds still reject those files."""
    import ctypes as C
    import subprocess
    import container_mutator as CM
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib_dir = os.path.join(root, "fpng_amd", "lib")
    dropin.shim()  # (builds the product libraries)
    so = os.path.join(lib_dir, "libfpng_test_nocrc.so")
    srcs = [os.path.join(root, "fpng_amd", "csrc", n) for n in ("fpng_dropin.cpp", "fpng_decode.cpp")] + [os.path.join(root, "tests", "cpp", "dropin_shim.cpp")]
    deps = srcs + [os.path.join(root, "fpng_amd", "csrc", "png_parse.h"), os.path.join(lib_dir, "libfpng_amd.so")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        # the CPU decoder + container walk with the switch on (in a process with a GPU, `python -m fpng_amd.build --variant nocrc`
        # builds libfpng_amd_nocrc.so + libfpng_nocrc.so so that the GPU tier's host side skips the CRCs as well)
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-DFPNG_DISABLE_DECODE_CRC32_CHECKS=1", "-I", os.path.join(root, "include"),
                               "-I", os.path.join(root, "fpng_amd", "csrc")] + srcs + ["-o", so, "-L", lib_dir, "-lfpng_amd", "-pthread", "-Wl,-rpath,$ORIGIN"])
    mine = C.CDLL(so)
    theirs = C.CDLL(os.path.join(root, "oracle", "_ref", "libfpng_ref_nocrc.so"))
    theirs.ref_init()

    def run(lib, prefix, f, desired):
        b = np.frombuffer(f, dtype=np.uint8)
        w, h, c = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        gst = getattr(lib, prefix + "_get_info")(C.c_void_p(b.ctypes.data), C.c_uint32(b.size), C.byref(w), C.byref(h), C.byref(c))
        if gst:
            return gst, None
        out = np.zeros(w.value * h.value * desired, dtype=np.uint8)
        st = getattr(lib, prefix + "_decode")(C.c_void_p(b.ctypes.data), C.c_uint32(b.size), C.c_void_p(out.ctypes.data), C.c_size_t(out.size),
                                              C.byref(w), C.byref(h), C.byref(c), C.c_uint32(desired))
        return st, (w.value, h.value, c.value, out.tobytes() if st == 0 else None)
    rng = np.random.default_rng(1212)
    accepted_only_without_checks = ihdr_still_checked = 0
    for _ in range(80):
        img, w, h, c = fuzz_image(rng)
        png = oracle().encode(img, w, h, c, int(rng.integers(0, 3)))
        chunks = CM.chunks_of(png)
        files = []
        for k in range(len(chunks)):  # one chunk's CRC damaged at a time (IHDR, fdEC, IDAT, IEND)
            ofs = 8 + sum(12 + len(body) for _, body in chunks[: k + 1]) - 1
            bad = bytearray(png)
            bad[ofs] ^= 0x5A
            files.append((chunks[k][0], bytes(bad)))
        for _ in range(6):  # flipped bits anywhere: with the checks off they reach the parser and the inflater
            bad = bytearray(png)
            for _ in range(int(rng.integers(1, 4))):
                bad[int(rng.integers(8, len(bad)))] ^= 1 << int(rng.integers(0, 8))
            files.append((b"bits", bytes(bad)))
        for name, f in files:
            desired = int(rng.choice([3, 4]))
            a, b = run(theirs, "ref", f, desired), run(mine, "shim", f, desired)
            assert a == b, (name, a[0], b[0])
            if name in (b"fdEC", b"IEND"):
                assert a[0] == 0 and ref().decode(f, desired)[0] == 4 and dropin.decode(f, desired)[0] == 4  # FPNG_DECODE_FAILED_HEADER_CRC32 by default
                accepted_only_without_checks += 1
            if name == b"IHDR":
                assert a[0] == 4
                ihdr_still_checked += 1
    assert accepted_only_without_checks >= 150 and ihdr_still_checked >= 80
