#!/usr/bin/env python
"""What a shard writer pays for a batch's files on the host, with scattered outputs and with a packed arena, on the same box.

    python tools/packed_timing.py [--form a|b|ab] [--repeats R] [--batches 512,1080p] [--package-root DIR]

Two batches (1024 x 512 x 512 RGB, 256 x 1080p RGB, grad / blocks contents), 1-pass, one submission each.  Two forms:
  a  today's: one output buffer of max_encoded_size() per image, wait() for the sizes, then one device-to-host copy per file into
     one pinned buffer, the files back to back
  b  packed:  submit_packed() into one arena (align 512, lead 512: a tar body), wait_packed(), ONE device-to-host copy of `total`
For both, per repeat: the GPU chain's time from device events around the submission (event, submit, join, event on the caller's
stream), and the host clock from the call of submit to the last byte on the host.  The forms take turns repeat by repeat; the
median is reported with its min-max, which is the spread the comparison has to be read against.  Form b's files are checked against
form a's before anything is timed.

--package-root DIR imports fpng_amd from another checkout (with its own built library), so that form a can be timed on the parent
commit's build in the same session: --form a --package-root <parent checkout>."""
import argparse
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--form", default="ab", choices=["a", "b", "ab"])
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--batches", default="512,1080p")
ap.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.package_root))
import fpng_amd  # noqa: E402  (before the first torch.cuda call: the library sets the hardware queue count)
import torch  # noqa: E402

BATCHES = {"512": (1024, 512, 512, 3), "1080p": (256, 1920, 1080, 3)}
ALIGN = LEAD = 512


def images(n, w, h, c):
    distinct = [torch.from_numpy(fpng_amd.synth_image("blocks" if i & 1 else "grad", w, h, c, seed=12345 + i)).cuda() for i in range(8)]
    return [distinct[i % 8] if i < 8 else distinct[i % 8].clone() for i in range(n)]


def run(enc, name, n, w, h, c):
    imgs = images(n, w, h, c)
    worst = fpng_amd.max_encoded_size(w, h, c)
    forms = {}
    pinned = torch.empty(n * (worst + 1024), dtype=torch.uint8, pin_memory=True)  # (one host buffer for both forms)
    if "a" in args.form:
        outs = [torch.empty(worst + 64, dtype=torch.uint8, device="cuda") for _ in range(n)]
        batch = enc.make_batch(imgs, outs)

        def form_a():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            enc.submit(batch)
            enc.join()
            e1.record()
            res = enc.wait(enc.last_ticket, n)
            pos = 0
            for out, (size, _, status) in zip(outs, res):
                assert status == 0
                pinned[pos:pos + size].copy_(out[:size], non_blocking=True)
                pos += size
            torch.cuda.synchronize()
            return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3, pos, [s for s, _, _ in res]
        forms["a"] = form_a
    if "b" in args.form:
        cap = fpng_amd.pack_capacity([(w, h, c)] * n, ALIGN, LEAD)
        raw = torch.empty(cap + ALIGN, dtype=torch.uint8, device="cuda")
        skip = (-raw.data_ptr()) % ALIGN
        arena = raw[skip:skip + cap]
        packed = enc.make_batch_packed(imgs)

        def form_b():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            enc.submit_packed(packed, arena, align=ALIGN, lead=LEAD)
            enc.join()
            e1.record()
            recs, total = enc.wait_packed(enc.last_ticket, n)
            pinned[:total].copy_(arena[:total], non_blocking=True)
            torch.cuda.synchronize()
            assert all(st == 0 for _, _, _, st in recs)
            return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3, total, recs
        forms["b"] = form_b
    # warm-up, and form b's files against form a's
    first, kept = {}, None
    for k, f in forms.items():
        first[k] = f()
        if k == "a" and len(forms) == 2:
            kept = pinned[:first[k][2]].clone()
    if kept is not None:
        pos = 0
        for size, (off, size_b, _, _) in zip(first["a"][3], first["b"][3]):
            assert size == size_b and torch.equal(kept[pos:pos + size], pinned[off:off + size]), "the packed files differ from the scattered ones"
            pos += size
        del kept
    for f in forms.values():
        f()
    t = {k: ([], []) for k in forms}
    for _ in range(args.repeats):
        for k, f in forms.items():
            gpu, host, _, _ = f()
            t[k][0].append(gpu), t[k][1].append(host)
    print(f"{name}: {n} x {w} x {h} x {c}, 1-pass, {args.repeats} repeats; median ms (min-max)", flush=True)
    for k in forms:
        g, hst = t[k]
        extra = f"output memory {n * (worst + 64) / 1e6:.0f} MB, {n} copies of {first[k][2] / 1e6:.1f} MB in all" if k == "a" else \
            f"arena {arena.numel() / 1e6:.0f} MB (the worst case; the files end at {first[k][2] / 1e6:.1f} MB), 1 copy"
        print(f"  form {k}: GPU chain {statistics.median(g):8.3f} ({min(g):.3f}-{max(g):.3f})   submit -> last byte on the host "
              f"{statistics.median(hst):8.3f} ({min(hst):.3f}-{max(hst):.3f})   {extra}", flush=True)
    if len(forms) == 2:
        ga, gb = statistics.median(t["a"][0]), statistics.median(t["b"][0])
        ha, hb = statistics.median(t["a"][1]), statistics.median(t["b"][1])
        spread = max((max(t[k][0]) - min(t[k][0])) / statistics.median(t[k][0]) for k in forms)
        print(f"  b / a: GPU chain {gb / ga:.3f} (largest min-max spread of the two: {100 * spread:.1f} %), host {hb / ha:.3f}", flush=True)


if __name__ == "__main__":
    enc = fpng_amd.Encoder(device=0)
    print(f"library: {fpng_amd._lib.LIB_PATH}   lanes {enc.lanes}", flush=True)
    for key in args.batches.split(","):
        run(enc, key, *BATCHES[key])
    enc.close()
