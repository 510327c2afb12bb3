"""Generate tests/golden/geometry.json from the UNMODIFIED reference (oracle/_ref/libfpng_ref.so): images whose FILE SIZES put the
encoder's last three kernels (scan, assemble or stored_*, finalize) into every cell of their geometry -- range size, farthest-range
sliver, tail padding, fold depth, stored block headers against the grid -- with size + sha256 of the reference's file.

Run where the reference build exists:   python oracle/make_golden_geometry.py

The geometry (tests/assemble_geometry.py, restated from fpng_amd/csrc/crc_geometry.h) depends on (w, h, c, file size, jobs of the
submission) only.  A stored file's size is a closed form of its dimensions: those cases are found by a search over (w, h, c).  A
compressed file's size is steered with the image's content: zeros whose first K pixels are seeded noise (assemble_geometry.case_image);
K is found by bisection for a target size and then stepped a pixel at a time (one more noise pixel adds 3 .. 11 bytes) until the
reference's file lies in the wanted cell.  The script fails if a planned cell finds no case.

  A  three submissions (flags 0, 1, 2: one submission has one mode) of GROUP_A_JOBS distinct jobs each, so that want = 4 binds: the
     planned cases below, then assemble_geometry.filler() jobs.  Compressed cases are raw images a little over 192 KiB (crc_blocks =
     5 > want); a forced-stored file that small reaches rl < 16 only as a small image, where crc_blocks (2) binds with want.
        rl 12 .. 16  x  sliver {0, 16, 32, 2^rl - 16, 2^(rl-1)}  x  mode;   pad 0 .. 15 x mode x c;   1, 2, 3, 4 ranges x mode;
        a 17 KB span (want says rl 13, crc_blocks alone 12)
  B  one job a submission, raw 64 .. 200 KiB, crc_blocks 3 / 4 / 5 decides rl: one case per rl and mode.  (Stored: rl 15 and 16
     only -- a stored file of a raw image of >= 64 KiB spans >= 65536 bytes, and rl <= 14 would need span < 16384 * crc_blocks with
     crc_blocks <= 5 reached only by raw images > 192 KiB.)
  C  one job a submission, fold depth: at every rl, n_ranges 256 | 257 (2048 x 2100 x 4), 512 | 513 (2048 x 4200 x 4) and
     1024 | 1025 (4096 x 4096 x 4, 64 MiB raw), 1-pass; one 2-pass (257 ranges) and one stored case per rl.  Every (rl, g) cell the
     rule reaches with at most 64 MiB raw is listed ("reachable_rl_g") and covered.
  S  stored walk, flags 2, one job a submission: n_filtered 65534 / 65535 / 65536 / 131070 / 131071; files of 6 blocks whose block-4
     header straddles only two pieces / a 4 KiB row / a range boundary, each with the neighbour one row taller; strides 4 .. 40 of
     both channel counts with two blocks, heights chosen so that filter bytes land at every piece offset and the fast path of
     assemble_stored meets col == 1, col + 16 == stride, every source misalignment and the image's last 16 bytes.

The file holds parameters and recorded results only: "cases" rows of "fields"; "cell" = [rl, n_ranges, g, pad, sliver] from the model."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import assemble_geometry as AG  # noqa: E402
from cpu_ref import have_ref, ref  # noqa: E402

FIELDS = ["name", "w", "h", "c", "seed", "noise_pixels", "flags", "group", "size", "sha256", "cell", "hits"]
MODES = {0: "1pass", 1: "2pass", 2: "stored"}
A4, A3 = (256, 192, 4), (256, 257, 3)  # group A's compressed images: crc_blocks = 5
C_IMAGES = {0: (2048, 2100, 4), 1: (2048, 2100, 4), 2: (2048, 4200, 4), 3: (4096, 4096, 4)}  # by fold depth g
MAX_RAW = 64 << 20


# ---------------------------------------------------------------------------------------------
# reference encodes of case_image(w, h, c, seed, K), with the work between neighbouring K kept small
# ---------------------------------------------------------------------------------------------
class Encodes:
    def __init__(self):
        self.key, self.img, self.noise, self.k, self.cache = None, None, None, 0, {}

    def png(self, w, h, c, seed, K, flags):
        import fpng_amd
        key = (w, h, c, seed)
        if key != self.key:
            self.key, self.k = key, 0
            self.img = np.zeros((h * w, c), dtype=np.uint8)
            self.noise = fpng_amd.synth_image("noise", w * h, 1, c, seed=seed).reshape(w * h, c)
        if K > self.k:
            self.img[self.k:K] = self.noise[self.k:K]
        else:
            self.img[K:self.k] = 0
        self.k = K
        return ref().encode(self.img, w, h, c, flags)

    def size(self, w, h, c, seed, K, flags):
        key = (w, h, c, seed, K, flags)
        if key not in self.cache:
            self.cache[key] = len(self.png(w, h, c, seed, K, flags))
        return self.cache[key]


ENC = Encodes()
USED = {}


def find_compressed(dims, flags, n_jobs, target_size, pred, seeds=range(1, 40), steps=400):
    """(seed, K, size) of the first image whose reference file is compressed and satisfies pred(Geometry, size)"""
    w, h, c = dims
    stored = AG.stored_size(w, h, c)
    for seed in seeds:
        lo, hi = 0, w * h
        while lo < hi:  # the least K whose file has target_size bytes or more (sizes grow with K, near enough)
            mid = (lo + hi) // 2
            if ENC.size(w, h, c, seed, mid, flags) >= target_size:
                hi = mid
            else:
                lo = mid + 1
        for K in range(max(lo - 3, 0), min(lo + steps, w * h) + 1):
            size = ENC.size(w, h, c, seed, K, flags)
            if size != stored and (seed, K) not in USED.setdefault((flags, w, h, c), set()) and pred(AG.geometry(w, h, c, size, n_jobs), size):
                USED[(flags, w, h, c)].add((seed, K))  # (every case is another image: the jobs of a submission are distinct)
                return seed, K, size
            if size > target_size + 4096:
                break
    raise SystemExit(f"no case for {dims} flags {flags} near {target_size} bytes")


# ---------------------------------------------------------------------------------------------
# the model over arrays of stored files
# ---------------------------------------------------------------------------------------------
def geometry_arrays(size, blocks, n_jobs):
    span = size - 16
    lim = np.minimum(AG.want_of(n_jobs), blocks)
    rl = 12 + sum(((span >> r) + 1 > lim).astype(np.int64) for r in range(12, 16))
    ea = (size - 20 + 15) & ~15
    n = (ea - 48 + (1 << rl) - 1) >> rl
    return dict(rl=rl, n_ranges=n, pad=ea - (size - 20), sliver=(ea - 48) & ((1 << rl) - 1), ea=ea, size=size)


def find_stored(pred, n_jobs, taken, wmax=420, hmax=420, cs=(3, 4), min_raw=0, max_raw=1 << 30):
    """the (w, h, c) of the fewest filtered bytes, not in `taken`, whose stored file satisfies pred(dict of arrays) -> mask"""
    best = None
    for c in cs:
        W, H = np.meshgrid(np.arange(1, wmax + 1, dtype=np.int64), np.arange(1, hmax + 1, dtype=np.int64))
        nf = (W * c + 1) * H
        size = 80 + nf + 5 * ((nf + 65534) // 65535)
        blocks = (size + 65535) // 65536 + 1
        a = geometry_arrays(size, blocks, n_jobs)
        a.update(w=W, h=H, c=c, nf=nf)
        mask = pred(a) & (W * H * c >= min_raw) & (W * H * c <= max_raw)
        ys, xs = np.nonzero(mask)
        for i in np.argsort(nf[ys, xs], kind="stable"):
            cand = (int(nf[ys[i], xs[i]]), int(W[ys[i], xs[i]]), int(H[ys[i], xs[i]]), c)
            if cand[1:] not in taken:
                best = cand if best is None or cand < best else best
                break
    if best is None:
        raise SystemExit("no stored image for a planned cell")
    taken.add(best[1:])
    return best[1:]


# ---------------------------------------------------------------------------------------------
CASES, STORED_TAKEN = [], set()


def add(group, dims, seed, K, flags, n_jobs, hits):
    w, h, c = dims
    png = ENC.png(w, h, c, seed, K, flags)
    geo = AG.geometry(w, h, c, len(png), n_jobs)
    name = "%s%d-%03d" % (group, flags, len(CASES))
    CASES.append([name, w, h, c, seed, K, flags, group, len(png), hashlib.sha256(png).hexdigest(), list(geo), hits])
    print(name, dims, "K", K, "size", len(png), geo, hits, flush=True)
    return geo


def add_stored(group, dims, n_jobs, hits):
    return add(group, dims, 77, dims[0] * dims[1], 2, n_jobs, hits)


def covered(group, flags):
    return [(r, AG.Geometry(*r[10])) for r in CASES if r[7] == group and r[6] == flags]


def span_window(rl, lim):
    """[lo, hi) of the spans that get range size 2^rl when min(want, crc_blocks) = lim"""
    return (0 if rl == 12 else lim << (rl - 1)), ((lim << rl) if rl < 16 else 1 << 40)


def group_a():
    n_jobs = AG.GROUP_A_JOBS
    assert AG.want_of(n_jobs) == 4 and AG.crc_blocks(*A4) == 5 and AG.crc_blocks(*A3) == 5
    for flags in (0, 1, 2):
        mode = MODES[flags]
        for rl in range(12, 17):
            for sliver in (0, 16, 32, (1 << rl) - 16, 1 << (rl - 1)):
                hits = "rl%d/s%d" % (rl, sliver)
                if flags == 2:
                    add_stored("A", find_stored(lambda a: (a["rl"] == rl) & (a["sliver"] == sliver), n_jobs, STORED_TAKEN), n_jobs, hits)
                    continue
                lo, hi = span_window(rl, 4)
                ea = next(48 + (m << rl) + sliver for m in range(0, 5) if 48 + (m << rl) + sliver - 11 >= max(lo, 2100) and 48 + (m << rl) + sliver + 4 < min(hi, 190000))
                seed, K, _ = find_compressed(A4, flags, n_jobs, ea + 5, lambda g, s: g.rl == rl and g.sliver == sliver)
                add("A", A4, seed, K, flags, n_jobs, hits)
        for n in (1, 2, 3, 4):
            if flags == 2:
                add_stored("A", find_stored(lambda a: a["n_ranges"] == n, n_jobs, STORED_TAKEN), n_jobs, "n%d" % n)
            else:
                seed, K, _ = find_compressed(A3, flags, n_jobs, (0, 0, 5000, 9500, 13500)[n], lambda g, s: g.n_ranges == n and g.rl == 12)
                add("A", A3, seed, K, flags, n_jobs, "n%d" % n)
        for c, dims in ((3, A3), (4, A4)):
            for pad in range(16):
                if any(g.pad == pad and r[3] == c for r, g in covered("A", flags)):
                    continue
                if flags == 2:
                    add_stored("A", find_stored(lambda a: a["pad"] == pad, n_jobs, STORED_TAKEN, cs=(c,), min_raw=1000), n_jobs, "pad%d" % pad)
                else:
                    seed, K, _ = find_compressed(dims, flags, n_jobs, 20000 + 1500 * pad, lambda g, s: g.pad == pad)
                    add("A", dims, seed, K, flags, n_jobs, "pad%d" % pad)
        if flags != 2:  # want = 4 says rl 13 where crc_blocks = 5 alone says 12
            pred = lambda g, s: 17000 <= s - 16 < 17400 and AG.range_log2(s - 16, n_jobs, 5) == 13 and AG.range_log2(s - 16, 1, 5) == 12  # noqa: E731
            seed, K, _ = find_compressed(A4, flags, n_jobs, 17100, pred)
            add("A", A4, seed, K, flags, n_jobs, "span17k")
    # coverage
    for flags in (0, 1, 2):
        got = covered("A", flags)
        for rl in range(12, 17):
            for sliver in (0, 16, 32, (1 << rl) - 16, 1 << (rl - 1)):
                assert any(g.rl == rl and g.sliver == sliver for _, g in got), (flags, rl, sliver)
        for c in (3, 4):
            assert {g.pad for r, g in got if r[3] == c} == set(range(16)), (flags, c)
        assert {1, 2, 3, 4} <= {g.n_ranges for _, g in got}, flags
        assert len(got) < n_jobs


def group_b():
    images = {3: (128, 128, 4), 4: (256, 129, 4), 5: A4}
    for b, d in images.items():
        assert AG.crc_blocks(*d) == b and (64 << 10) <= d[0] * d[1] * d[2] <= (200 << 10)
    plan = {12: 4, 13: 5, 14: 3, 15: 4, 16: 5}
    for flags in (0, 1):
        for rl, b in plan.items():
            lo, hi = span_window(rl, b)
            hi = min(hi, AG.stored_size(*images[b]) - 3000)
            seed, K, _ = find_compressed(images[b], flags, 1, max((lo + hi) // 2, 2000), lambda g, s: g.rl == rl)
            geo = add("B", images[b], seed, K, flags, 1, "rl%d/cb%d" % (rl, b))
            assert geo.rl == rl and AG.range_log2(CASES[-1][8] - 16, 1, 1 << 20) == 12  # (want alone would say 12: crc_blocks decides)
    for rl in (15, 16):
        dims = find_stored(lambda a: a["rl"] == rl, 1, STORED_TAKEN, min_raw=64 << 10, max_raw=200 << 10)
        add_stored("B", dims, 1, "rl%d/cb%d" % (rl, AG.crc_blocks(*dims)))
    for flags in (0, 1, 2):
        want = {15, 16} if flags == 2 else set(range(12, 17))
        assert {g.rl for _, g in covered("B", flags)} == want
    # stored, rl <= 14: span >= 65536 + 60 would have to be < 16384 * crc_blocks, crc_blocks <= 4 for a raw image of at most 192 KiB,
    # and a raw image over 192 KiB spans more than 5 * 16384
    for b, raw_least in ((3, 64 << 10), (4, 128 << 10), (5, 192 << 10)):
        assert raw_least + 60 >= (b << 14)


def reachable_rl_g():
    """every (rl, g) the rule gives some file of some image of at most 64 MiB raw, one job a submission"""
    cells = set()
    blocks_most = AG.crc_blocks(4096, 4096, 4)
    assert 4096 * 4096 * 4 == MAX_RAW
    b = np.arange(2, blocks_most + 1, dtype=np.int64)
    for rl in range(12, 17):
        for n in range(1, (MAX_RAW >> rl) + 3):
            for span in (48 + (n << rl) + 4, 48 + ((n - 1) << rl) + 16 + 4):  # n full ranges | the farthest one of 16 bytes; pad 0
                ok = (span + 16 <= (b - 1) * 65536) & (((span >> rl) + 1 <= np.minimum(2048, b)) | (rl == 16))
                if rl > 12:
                    ok &= (span >> (rl - 1)) + 1 > np.minimum(2048, b)
                if ok.any():
                    got = AG.rule(span, 1, int(b[ok][0]))
                    assert got[0] == rl and got[1] == n, (span, got)
                    cells.add((rl, got[2]))
    return sorted(cells)


def group_c():
    reach = reachable_rl_g()
    print("reachable (rl, g):", reach)
    assert reach == [(rl, g) for rl in range(12, 17) for g in range(4)], reach
    for g in (1, 2, 3):
        dims = C_IMAGES[g]
        assert dims[0] * dims[1] * dims[2] <= MAX_RAW
        for rl in range(12, 17):
            for n in (256 << (g - 1), (256 << (g - 1)) + 1):
                ea = 48 + ((256 << (g - 1)) << rl) + (16 if n & 1 else 0)  # the farthest range full | 16 bytes of one more
                hits = "rl%d/n%d" % (rl, n)
                try:
                    seed, K, _ = find_compressed(dims, 0, 1, ea + 5, lambda q, s: q.rl == rl and q.n_ranges == n and end_ok(s, ea), seeds=range(1, 6), steps=60)
                    add("C", dims, seed, K, 0, 1, hits)
                except SystemExit:
                    # (the reference stores what does not compress: the stored file of this image, if it is in the cell)
                    geo = AG.geometry(*dims, AG.stored_size(*dims), 1)
                    assert geo.rl == rl and geo.n_ranges == n, (hits, geo)
                    add_stored("C", dims, 1, hits + "/fallback")
    for rl in range(12, 17):
        ea = 48 + (256 << rl) + 16
        seed, K, _ = find_compressed(C_IMAGES[1], 1, 1, ea + 5, lambda q, s: q.rl == rl and q.n_ranges == 257, seeds=range(1, 6), steps=60)
        add("C", C_IMAGES[1], seed, K, 1, 1, "rl%d/2pass" % rl)
        if rl < 16:
            dims = find_stored(lambda a: (a["rl"] == rl) & (a["sliver"] == 16), 1, STORED_TAKEN)
        else:  # a stored file of 257 ranges: the smallest 2048-pixel-wide image that has them
            dims = next((2048, h, 4) for h in range(2040, 2110) if AG.geometry(2048, h, 4, AG.stored_size(2048, h, 4), 1)[:3] == (16, 257, 1))
        add_stored("C", dims, 1, "rl%d/stored" % rl)
    got = {(g.rl, g.g) for fl in (0, 1, 2) for _, g in covered("C", fl)}
    assert got >= set(reach), sorted(set(reach) - got)
    for fl in (1, 2):
        assert {g.rl for _, g in covered("C", fl)} >= set(range(12, 17))
    return reach


def end_ok(size, ea):
    return AG.end_aligned_of(size) == ea


def group_s():
    def dims_of(nf):
        for stride in range(4, nf + 1):
            if nf % stride == 0:
                for c in (3, 4):
                    if (stride - 1) % c == 0 and (stride - 1) // c <= 1 << 16:
                        return (stride - 1) // c, nf // stride, c
        raise SystemExit(f"no image of {nf} filtered bytes")
    for nf in (65534, 65535, 65536, 131070, 131071):
        d = (64, 255, 4) if nf == 65535 else (5, 4096, 3) if nf == 65536 else dims_of(nf)
        assert AG.n_filtered(*d) == nf
        add_stored("S", d, 1, "nf%d" % nf)
    # six blocks, the header of block 4 at file offset 262220 = 12 mod 16
    six = lambda a: (a["nf"] > 5 * 65535) & (a["nf"] <= 6 * 65535) & (a["rl"] == 16)  # noqa: E731
    row = lambda a: (a["ea"] - 262224) % 4096 == 0  # noqa: E731
    rng = lambda a: (a["ea"] - 262224) % 65536 == 0  # noqa: E731
    for what, pred in (("piece", lambda a: six(a) & ~row(a)), ("row", lambda a: six(a) & row(a) & ~rng(a)), ("range", lambda a: six(a) & rng(a))):
        w, h, c = find_stored(pred, 1, STORED_TAKEN, wmax=2000, hmax=2000)
        assert AG.header_class(w, h, c) == what, (what, w, h, c, AG.header_class(w, h, c))
        add_stored("S", (w, h, c), 1, "hdr4/" + what)
        if what != "piece":
            assert AG.header_class(w, h + 1, c) == "piece", (what, w, h + 1, c)
            add_stored("S", (w, h + 1, c), 1, "hdr4/" + what + "+1row")
    # strides 4 .. 40
    need = {"off%d" % o for o in range(16)} | {"col1", "col_end", "last16"} | {"m%d" % q for q in range(4)}

    def items(w, h, c):
        walk = AG.stored_walk(w, h, c)
        p = walk["pieces"]
        return {"off%d" % o for o in walk["filter_piece_offsets"]} | ({"col1"} if p["col1"] else set()) | ({"col_end"} if p["col_end"] else set()) | \
            ({"last16"} if p["last16"] else set()) | {"m%d" % q for q in range(4) if p["m"][q]}
    have = set()
    for c in (3, 4):
        for w in range(1, 14):
            stride = w * c + 1
            if not 4 <= stride <= 40:
                continue
            h0 = 65535 // stride + 1
            h = max(range(h0, h0 + 48), key=lambda q: (len(items(w, q, c) - have), -q))
            assert AG.stored_blocks(w, h, c) == 2
            got = items(w, h, c)
            add_stored("S", (w, h, c), 1, "stride%d" % stride + ("/last16" if "last16" in got else ""))
            have |= got
    assert have == need, sorted(need - have)
    assert {r[1] * r[3] + 1 for r in CASES if r[7] == "S" and r[11].startswith("stride")} == {s for s in range(4, 41) if (s - 1) % 3 == 0 or (s - 1) % 4 == 0}


def fillers():
    out = {}
    for flags in (0, 1, 2):
        n = AG.GROUP_A_JOBS - len(covered("A", flags))
        total, shas, seen = 0, [], {tuple(r[1:6]) for r in CASES if r[7] == "A" and r[6] == flags}
        for i in range(n):
            w, h, c, seed, K = AG.filler(flags, i)
            assert (w, h, c, seed, K) not in seen
            seen.add((w, h, c, seed, K))
            png = ref().encode(AG.case_image(w, h, c, seed, K), w, h, c, flags)
            total += len(png)
            shas.append(hashlib.sha256(png).hexdigest())
        out[str(flags)] = {"n": n, "total_size": total, "sha256_all": hashlib.sha256("".join(shas).encode()).hexdigest()}
    return out


def main():
    assert have_ref(), "oracle/_ref/libfpng_ref.so is missing (make -C oracle, where the reference's sources are at hand)"
    group_a()
    group_b()
    reach = group_c()
    group_s()
    out = {"fields": FIELDS, "group_a_jobs": AG.GROUP_A_JOBS, "fillers": fillers(), "reachable_rl_g": [list(v) for v in reach], "cases": CASES}
    path = os.path.join(ROOT, "tests", "golden", "geometry.json")
    with open(path, "w") as f:
        f.write("{\n")
        for k in ("fields", "group_a_jobs", "fillers", "reachable_rl_g"):
            f.write(json.dumps(k) + ": " + json.dumps(out[k], separators=(",", ":")) + ",\n")
        f.write('"cases": [\n' + ",\n".join(json.dumps(r, separators=(",", ":")) for r in CASES) + "\n]\n}\n")
    limit = sum(os.path.getsize(os.path.join(ROOT, "tests", "golden", n)) for n in ("kat.json", "batches.json"))
    assert os.path.getsize(path) < limit, (os.path.getsize(path), limit)
    print("wrote tests/golden/geometry.json:", len(CASES), "cases,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
