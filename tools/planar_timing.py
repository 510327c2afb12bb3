#!/usr/bin/env python
"""What the planar (CHW) entry points cost against the packed ones, and against what a CHW caller did before them -- a permute copy
in front of every encode and behind every decode -- on the same box in one process.

    python tools/planar_timing.py [rounds] [steps]

Two workloads (8 x 8K RGBA grad, 256 x 1080p RGB grad), encode and decode each.  The variants take turns round by round; a window is
`steps` back-to-back steps (encode: submissions of the whole batch over four output sets, timed with device events as
tools/layout_timing.py does; decode: calls on a descriptor built once, timed on the host clock as tools/decode_layout_timing.py
does); the median window is reported per step with its min-max.  Variants:
  encode   a  packed HWC through submit          p  CHW through submit_planar
           c  dst.copy_(chw.permute(1, 2, 0)) into a preallocated HWC tensor, then a
  decode   a  packed decode_device               p  decode_device_planar into CHW
           c  a, then dst.copy_(hwc.permute(2, 0, 1))
Every variant's output is checked first (encode: the packed path's files; decode: the packed path's pixels permuted).
The last line of every block says whether p beat c with min-max ranges that do not overlap (the gate), and p / a."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fpng_amd  # noqa: E402  (before the first torch.cuda call: the library sets the hardware queue count)
import torch  # noqa: E402

SETS = 4


def report(name, what, t, n, w, h):
    print(f"{name}, {what}: median ms per step (min-max), relative to a", flush=True)
    base = statistics.median(t["a"])
    for key in t:
        m = statistics.median(t[key])
        print(f"  {key:3s} {m:8.4f} ms ({min(t[key]):.4f}-{max(t[key]):.4f})  {m / base:6.3f}  {n * w * h / m / 1e6:7.1f} GP/s", flush=True)
    ok = max(t["p"]) < min(t["c"])
    print(f"  gate p < c, ranges apart: {'PASSED' if ok else 'MISSED'}   p / c = {statistics.median(t['p']) / statistics.median(t['c']):.3f}   "
          f"p / a = {statistics.median(t['p']) / base:.3f}", flush=True)
    return ok


def encode(enc, name, w, h, c, n, rounds, steps):
    hwc = [torch.from_numpy(fpng_amd.synth_image("grad", w, h, c, seed=12345 + i)).cuda() for i in range(n)]
    chw = [im.permute(2, 0, 1).contiguous() for im in hwc]
    tmp = [[torch.empty_like(im) for im in hwc] for _ in range(SETS)]
    outs = [[torch.empty(fpng_amd.max_encoded_size(w, h, c) + 64, dtype=torch.uint8, device="cuda") for _ in range(n)] for _ in range(SETS)]
    planar = [enc.make_batch_planar(chw, outs[k]) for k in range(SETS)]
    packed = [enc.make_batch(hwc, outs[k]) for k in range(SETS)]
    copied = [enc.make_batch(tmp[k], outs[k]) for k in range(SETS)]

    def sub_a(k):
        enc.submit(packed[k])

    def sub_p(k):
        enc.submit_planar(planar[k])

    def sub_c(k):
        for src, dst in zip(chw, tmp[k]):
            dst.copy_(src.permute(1, 2, 0))
        enc.submit(copied[k])
    v = {"a": sub_a, "p": sub_p, "c": sub_c}

    def window(fn, m):
        tickets = [None] * SETS
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for s in range(m):
            k = s % SETS
            if tickets[k] is not None:
                enc.wait(tickets[k], n)  # (this output set's previous submission: done before its buffers are written again)
            fn(k)
            tickets[k] = enc.last_ticket
        enc.join()
        e1.record()
        e1.synchronize()
        enc.finish(n)
        return e0.elapsed_time(e1) / m
    ref = None
    for key, fn in v.items():  # the files first
        for o in outs[0]:
            o.zero_()
        window(fn, 1)
        res = enc.finish(n)
        got = [(r[0], fpng_amd.fpng_crc32(outs[0][i][:r[0]].cpu().numpy())) for i, r in enumerate(res)]
        ref = ref or got
        assert got == ref, f"{name}: encode variant {key} wrote other files than the packed path"
    for fn in v.values():
        window(fn, 4)
    t = {key: [] for key in v}
    for _ in range(rounds):
        for key, fn in v.items():
            t[key].append(window(fn, steps))
    return report(name, f"encode, {rounds} rounds x {steps} steps", t, n, w, h)


def decode(enc, name, w, h, c, n, rounds, steps):
    pngs = []
    for i in range(4):
        (p,), _ = enc.encode_tensors([torch.from_numpy(fpng_amd.synth_image("grad", w, h, c, seed=12345 + i)).cuda()], 0)
        pngs.append(p)
    dev = [torch.frombuffer(bytearray(pngs[i % 4]), dtype=torch.uint8).cuda() for i in range(n)]
    packed = enc.make_decode_batch(dev, c, [(w, h)] * n)
    nchw = torch.empty((n, c, h, w), dtype=torch.uint8, device="cuda")
    tmp = torch.empty((n, c, h, w), dtype=torch.uint8, device="cuda")
    planar = enc.make_decode_batch_planar(dev, list(nchw))

    def dec_c():
        enc.decode_device(packed, results=False)
        for src, dst in zip(packed.outs, tmp):
            dst.copy_(src.view(h, w, c).permute(2, 0, 1))
        torch.cuda.synchronize()
    v = {"a": lambda: enc.decode_device(packed, results=False), "p": lambda: enc.decode_device_planar(planar, results=False), "c": dec_c}
    for fn in v.values():
        fn()
    assert all(s == 0 for s in packed.statuses()) and all(s == 0 for s in planar.statuses())
    for i, p in enumerate(packed.outs):
        want = p.view(h, w, c).permute(2, 0, 1)
        assert torch.equal(nchw[i], want) and torch.equal(tmp[i], want), f"{name}: a decode variant wrote other pixels than the packed path"

    def window(fn, m):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(m):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / m
    for fn in v.values():
        window(fn, 3)
    t = {key: [] for key in v}
    for _ in range(rounds):
        for key, fn in v.items():
            t[key].append(window(fn, steps))
    return report(name, f"decode, {rounds} rounds x {steps} calls", t, n, w, h)


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    enc = fpng_amd.Encoder(device=0)
    ok = True
    for args in (("8 x 8K RGBA grad", 7680, 4320, 4, 8), ("256 x 1080p RGB grad", 1920, 1080, 3, 256)):
        for fn in (encode, decode):
            ok &= fn(enc, *args, rounds, steps)
            torch.cuda.empty_cache()
    enc.close()
    print("gate (p faster than c in all four, ranges apart):", "PASSED" if ok else "MISSED")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
