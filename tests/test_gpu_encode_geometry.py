"""GPU tests (-m gpu) of the encoder's last three kernels -- scan, assemble (or stored_*), finalize -- over FILE SIZES.

How those kernels divide a file depends on its size, the jobs of the submission and the image's maximum size, never on its content
(fpng_amd/csrc/crc_geometry.h; assemble_geometry.py restates it).  tests/golden/geometry.json (oracle/make_golden_geometry.py) holds
images whose reference files lie in every cell of that geometry: every range size with the farthest range full, 16 and 32 bytes,
one piece short and half; every tail padding; 1 .. 4 ranges; 256 | 257, 512 | 513 and 1024 | 1025 ranges at every range size (the
fold's depth); stored block headers across pieces, 4 KiB rows and ranges; stored strides 4 .. 40.  The judge is the reference's file
as size + sha256 (with the reference build at hand a mismatch names the first differing byte).  Every output lies in a buffer of
sentinel bytes: behind png_size rounded up to 16 nothing may be written.  The files then go through the decoder with its CRC-32 and
Adler-32 checks on, from addresses of every residue mod 16: the same sweep for dec_crc_kernel / dec_verify_kernel."""
import hashlib
import json
import os

import numpy as np
import pytest

import assemble_geometry as AG
from cpu_ref import have_ref, ref

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "geometry.json")) as _f:
    FIX = json.load(_f)
CASES = [dict(zip(FIX["fields"], row)) for row in FIX["cases"]]


def _cases(group, flags=None):
    return [k for k in CASES if k["group"] == group and (flags is None or k["flags"] == flags)]


@pytest.fixture(scope="module")
def enc(built_lib):
    import torch
    import fpng_amd
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    e = fpng_amd.Encoder(device=0)
    e.set_decode_verify(fpng_amd.VERIFY_CRC32 | fpng_amd.VERIFY_ADLER32)
    yield e
    e.close()


def _image(k):
    return AG.case_image(k["w"], k["h"], k["c"], k["seed"], k["noise_pixels"])


def _up(v, a):
    return -(-v // a) * a


def _slots(dims):
    """one sentinel-filled device buffer with a slot of max_encoded_size + 64 bytes (256-byte aligned) per image -> (buffer, offsets, slot sizes)"""
    import torch
    caps = [_up(AG.max_encoded_size(w, h, c) + 64, 256) for w, h, c in dims]
    offs = np.concatenate([[0], np.cumsum(caps)]).tolist()
    buf = torch.full((offs[-1],), SENTINEL, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 256 == 0
    return buf, offs[:-1], caps


def _first_difference(png, img, flags):
    if not have_ref():
        return ""
    h, w, c = img.shape
    exp = ref().encode(img, w, h, c, flags)
    n = min(len(png), len(exp))
    x = np.frombuffer(png[:n], np.uint8) != np.frombuffer(exp[:n], np.uint8)
    return f"; the reference's file has {len(exp)} bytes, first difference at byte {int(np.argmax(x)) if x.any() else n}"


def _check_file(host, off, cap, size, want_size, want_sha, what, img, flags):
    """the file at host[off:off + size] against the recorded answer; the slot behind the file's last 16-byte piece against the sentinel"""
    png = host[off:off + size].tobytes()
    ok = size == want_size and (want_sha is None or hashlib.sha256(png).hexdigest() == want_sha)
    assert ok, f"{what}: {size} bytes, recorded {want_size}" + ("" if size != want_size else ", another sha256") + _first_difference(png, img, flags)
    tail = host[off + _up(size, 16):off + cap]
    bad = np.flatnonzero(tail != SENTINEL)
    assert not bad.size, f"{what}: byte {_up(size, 16) + int(bad[0])} behind the file ({size} bytes) was written"
    return png


def _submit(enc, path, imgs, flags):
    """one submission of the images (h, w, c) through `path` -> (buffer, offsets, caps, sizes, the source tensors)"""
    import torch
    dims = [(im.shape[1], im.shape[0], im.shape[2]) for im in imgs]
    buf, offs, caps = _slots(dims)
    outs = [buf[o:o + cp] for o, cp in zip(offs, caps)]
    if path == "submit":
        src = [torch.from_numpy(im).cuda() for im in imgs]
        n = enc.submit(src, outs, flags)
    elif path == "ex":  # B,G,R[,A] with a padded pitch
        src = []
        for im in imgs:
            h, w, c = im.shape
            wide = np.full((h, w + 3, c), 0x5A, dtype=np.uint8)
            wide[:, :w, :] = im[..., [2, 1, 0] + ([3] if c == 4 else [])]
            src.append(torch.from_numpy(wide).cuda()[:, :w, :])
        n = enc.submit_ex(src, outs, flags, order="bgr")
    elif path == "planar":
        src = [torch.from_numpy(np.ascontiguousarray(im.transpose(2, 0, 1))).cuda() for im in imgs]
        n = enc.submit_planar(src, outs, flags)
    else:  # f16 planes whose values quantise back to the bytes: |half(b / 255) * 255 - b| <= 255 * 2^-11 < 1/2
        src = [(torch.from_numpy(np.ascontiguousarray(im.transpose(2, 0, 1))).cuda().to(torch.float32) / 255.0).to(torch.float16) for im in imgs]
        for s, im in zip(src[:2], imgs[:2]):
            assert np.array_equal((s.to(torch.float32) * 255.0).round().to(torch.uint8).cpu().numpy(), im.transpose(2, 0, 1))
        n = enc.submit_float(src, outs, flags)
    res = enc.wait(enc.last_ticket, n)
    assert n == len(imgs) and all(st == 0 for _, _, st in res), [r for r in res if r[2]][:4]
    if flags & 2:
        assert all(mode == 1 for _, mode, _ in res)
    return buf, offs, caps, [int(r[0]) for r in res], src


def _round_trip(enc, host_files, imgs, first_index=0):
    """the files through decode_device with both checks on, from addresses whose residue mod 16 is (case index) mod 16"""
    import torch
    for c in (3, 4):
        idx = [i for i, im in enumerate(imgs) if im.shape[2] == c]
        if not idx:
            continue
        offs, at = [], 0
        for i in idx:
            at = _up(at, 16) + (first_index + i) % 16
            offs.append(at)
            at += len(host_files[i]) + 16
        flat = np.full(at + 16, SENTINEL, dtype=np.uint8)
        for i, o in zip(idx, offs):
            flat[o:o + len(host_files[i])] = np.frombuffer(host_files[i], np.uint8)
        dev = torch.from_numpy(flat).cuda()
        assert dev.data_ptr() % 16 == 0
        pngs = [dev[o:o + len(host_files[i])] for i, o in zip(idx, offs)]
        res = enc.decode_device(pngs, c, [(imgs[i].shape[1], imgs[i].shape[0]) for i in idx])
        for i, o, (status, px, chans) in zip(idx, offs, res):
            assert status == 0 and chans == c, f"file {first_index + i} at residue {o % 16}: decode status {status}"
            assert torch.equal(px.cpu(), torch.from_numpy(imgs[i])), f"file {first_index + i} at residue {o % 16}: the decoded pixels differ from the source"


def _model_holds(k, n_jobs):
    """the cell the fixture lists is the cell the model computes: a change of the rule says so here"""
    geo = AG.geometry(k["w"], k["h"], k["c"], k["size"], n_jobs)
    assert list(geo) == k["cell"], f"{k['name']} ({k['hits']}): the fixture says {k['cell']}, the model {list(geo)}"
    return geo


# ---------------------------------------------------------------------------------------------
# group A: GROUP_A_JOBS jobs in ONE submission (per mode: a submission has one set of flags), so that want = 4 binds
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, 1, 2])
def test_group_a_one_submission_of_many_small_jobs(enc, flags):
    import fpng_amd
    planned = _cases("A", flags)
    fill = FIX["fillers"][str(flags)]
    n_jobs = len(planned) + fill["n"]
    assert n_jobs == FIX["group_a_jobs"] == AG.GROUP_A_JOBS >= 520 and AG.want_of(n_jobs) == 4
    geos = [_model_holds(k, n_jobs) for k in planned]
    for rl in range(12, 17):
        for sliver in (0, 16, 32, (1 << rl) - 16, 1 << (rl - 1)):
            assert any(g.rl == rl and g.sliver == sliver for g in geos), (rl, sliver)
    for c in (3, 4):
        assert {g.pad for k, g in zip(planned, geos) if k["c"] == c} == set(range(16))
    assert {1, 2, 3, 4} <= {g.n_ranges for g in geos}
    if flags != 2:  # compressed: raw images a little over 192 KiB, and one file where want and crc_blocks alone disagree
        assert all(AG.crc_blocks(k["w"], k["h"], k["c"]) == 5 for k in planned)
        assert any(AG.range_log2(k["size"] - 16, n_jobs, 5) != AG.range_log2(k["size"] - 16, 1, 5) for k in planned if k["hits"] == "span17k")
    imgs = [_image(k) for k in planned] + [AG.case_image(*AG.filler(flags, i)) for i in range(fill["n"])]
    assert len({(im.shape, im.tobytes()) for im in imgs}) == n_jobs  # distinct jobs

    def check(get, sizes, what):
        files = []
        for i, k in enumerate(planned):
            files.append(get(i, sizes[i], k["size"], k["sha256"], f"{what} {k['name']} ({k['hits']})"))
        shas = []
        for i in range(len(planned), n_jobs):
            files.append(get(i, sizes[i], sizes[i], None, f"{what} filler {i - len(planned)}"))
            shas.append(hashlib.sha256(files[-1]).hexdigest())
        assert sum(sizes[len(planned):]) == fill["total_size"], f"{what}: the fillers' sizes"
        if hashlib.sha256("".join(shas).encode()).hexdigest() != fill["sha256_all"]:
            bad = [i for i in range(len(planned), n_jobs) if have_ref() and files[i] != ref().encode(imgs[i], imgs[i].shape[1], imgs[i].shape[0], imgs[i].shape[2], flags)]
            raise AssertionError(f"{what}: the fillers' files differ from the reference's" + (f": fillers {[i - len(planned) for i in bad][:8]}" if bad else ""))
        return files

    # one submission
    buf, offs, caps, sizes, src = _submit(enc, "submit", imgs, flags)
    host = buf.cpu().numpy()
    files = check(lambda i, size, ws, sha, what: _check_file(host, offs[i], caps[i], size, ws, sha, what, imgs[i], flags), sizes, f"flags {flags}")

    # the same jobs into one packed arena: the heads are pack_heads_kernel's
    import torch
    align, lead = 16, 512
    cap = fpng_amd.pack_capacity([(im.shape[1], im.shape[0], im.shape[2]) for im in imgs], align, lead)
    arena = torch.full((cap + 4096,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert arena.data_ptr() % 16 == 0
    assert enc.submit_packed(src, arena[:cap], align=align, lead=lead, flags=flags) == n_jobs
    recs, total = enc.wait_packed(enc.last_ticket, n_jobs)
    want_place, want_total = fpng_amd.pack_place(sizes, align, lead, cap)
    assert [(r[0], r[3]) for r in recs] == [tuple(p) for p in want_place] and total == want_total and all(r[3] == 0 for r in recs)
    ahost = arena.cpu().numpy()
    untouched = np.ones(ahost.size, dtype=bool)
    for off, size, _, _ in recs:
        untouched[off:off + _up(size, 16)] = False
    assert (ahost[untouched] == SENTINEL).all(), "packed: bytes outside the files were written"
    packed = check(lambda i, size, ws, sha, what: _check_file(ahost, recs[i][0], _up(size, 16), size, ws, sha, what, imgs[i], flags), [r[1] for r in recs], f"packed flags {flags}")
    assert packed == files

    _round_trip(enc, files, imgs)


# ---------------------------------------------------------------------------------------------
# groups B, C, S: one job per submission
# ---------------------------------------------------------------------------------------------
def _one_by_one(enc, cases, paths=("submit",), round_trip=True):
    out = []
    for index, k in enumerate(cases):
        geo = _model_holds(k, 1)
        img = _image(k)
        first = None
        for path in paths:
            buf, offs, caps, sizes, _ = _submit(enc, path, [img], k["flags"])
            png = _check_file(buf.cpu().numpy(), 0, caps[0], sizes[0], k["size"], k["sha256"], f"{k['name']} ({k['hits']}) {geo} via {path}", img, k["flags"])
            first = png if first is None else first
            assert png == first
        if round_trip:
            _round_trip(enc, [first], [img], first_index=index)
        out.append(geo)
    return out


def test_group_b_crc_blocks_decides_the_range_size(enc):
    cases = _cases("B")
    for k in cases:
        assert (64 << 10) <= k["w"] * k["h"] * k["c"] <= (200 << 10) and AG.crc_blocks(k["w"], k["h"], k["c"]) in (3, 4, 5)
        span = k["size"] - 16  # one job: want = 2048 leaves the choice to crc_blocks
        assert AG.range_log2(span, 1, 1 << 20) == 12 and AG.range_log2(span, 1, AG.crc_blocks(k["w"], k["h"], k["c"])) == k["cell"][0]
    for flags, want in ((0, {12, 13, 14, 15, 16}), (1, {12, 13, 14, 15, 16}), (2, {15, 16})):
        assert {k["cell"][0] for k in cases if k["flags"] == flags} == want
    _one_by_one(enc, cases, round_trip=False)


@pytest.mark.parametrize("part", ["256|257", "512|513", "1024|1025", "2-pass and stored"])
def test_group_c_fold_depth(enc, part):
    """n_ranges on both sides of each step of the fold's depth g, at every range size; the largest input is one 64 MiB image"""
    all_c = _cases("C")
    reach = {tuple(v) for v in FIX["reachable_rl_g"]}
    assert reach == {(rl, g) for rl in range(12, 17) for g in range(4)} and {(k["cell"][0], k["cell"][2]) for k in all_c} >= reach
    assert max(k["w"] * k["h"] * k["c"] for k in all_c) == 64 << 20
    if part[0].isdigit() and "|" in part:
        lo = int(part.split("|")[0])
        cases = [k for k in all_c if k["hits"].split("/")[1] in ("n%d" % lo, "n%d" % (lo + 1))]
        assert sorted((k["cell"][0], k["cell"][1]) for k in cases) == [(rl, n) for rl in range(12, 17) for n in (lo, lo + 1)]
    else:
        cases = [k for k in all_c if k["hits"].split("/")[1] in ("2pass", "stored")]
        for flags in (1, 2):
            assert {k["cell"][0] for k in cases if k["flags"] == flags} == set(range(12, 17))
    geos = _one_by_one(enc, cases)
    assert all(g.g == AG.rule(k["size"] - 16, 1, AG.crc_blocks(k["w"], k["h"], k["c"]))[2] for g, k in zip(geos, cases))


def test_group_s_stored_walk_through_every_stored_kernel(enc):
    """assemble_kernel's stored branch and stored_kernel's _ex, planar and planar float (f32) instantiations write the same files"""
    cases = _cases("S")
    assert all(k["flags"] == 2 for k in cases)
    assert {AG.n_filtered(k["w"], k["h"], k["c"]) for k in cases} >= {65534, 65535, 65536, 131070, 131071}
    classes = {k["hits"]: AG.header_class(k["w"], k["h"], k["c"]) for k in cases if k["hits"].startswith("hdr4/")}
    assert classes == {"hdr4/piece": "piece", "hdr4/row": "row", "hdr4/row+1row": "piece", "hdr4/range": "range", "hdr4/range+1row": "piece"}
    for k in cases:
        if k["hits"].startswith("hdr4/"):
            assert AG.stored_blocks(k["w"], k["h"], k["c"]) >= 6 and 262220 + 5 < k["size"] - 20
    strides = [k for k in cases if k["hits"].startswith("stride")]
    assert {k["w"] * k["c"] + 1 for k in strides if k["c"] == 3} == set(range(4, 41, 3)) and {k["w"] * k["c"] + 1 for k in strides if k["c"] == 4} == set(range(5, 41, 4))
    offsets, col1, col_end, last16, m = set(), 0, 0, 0, [0] * 4
    for k in strides:
        walk = AG.stored_walk(k["w"], k["h"], k["c"])
        assert len(walk["headers"]) >= 2
        offsets |= set(walk["filter_piece_offsets"])
        p = walk["pieces"]
        col1, col_end, last16, m = col1 + p["col1"], col_end + p["col_end"], last16 + p["last16"], [a + b for a, b in zip(m, p["m"])]
    assert offsets == set(range(16)) and col1 and col_end and last16 and all(m)
    _one_by_one(enc, cases, paths=("submit", "ex", "planar", "float"))
