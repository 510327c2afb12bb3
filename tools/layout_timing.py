#!/usr/bin/env python
"""Cost of a source layout (Encoder.submit_ex) against the packed path and against repacking first, on the same box in one process.

    python tools/layout_timing.py [rounds] [steps]

Per workload (8 x 8K RGBA grad, 256 x 1080p RGB grad) and variant, a window of `steps` back-to-back submissions of the whole batch
(four output sets, so that up to four are in flight as in bench.py), timed with device events on torch's stream; the variants take
turns round by round and the median window is reported per step.  Variants:
  a  packed RGBA through submit                 b  BGRA, pitch w*4 + 256, through submit_ex
  c  BGRA -> RGBA copy (the channel gather + contiguous), then a
  d  packed RGB through submit                  e1 BGR through submit_ex      e2 RGBX (4-byte pixels) through submit_ex
  f  [..., :3].contiguous() of the RGBX buffer, then d
Every variant's files are checked against variant a / d first."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fpng_amd  # noqa: E402  (before the first torch.cuda call: the library sets the hardware queue count)
import torch  # noqa: E402

SETS = 4


def workload(name, w, h, c, n):
    imgs = [torch.from_numpy(fpng_amd.synth_image("grad", w, h, c, seed=12345 + i)).cuda() for i in range(n)]
    outs = [[torch.empty(fpng_amd.max_encoded_size(w, h, c) + 64, dtype=torch.uint8, device="cuda") for _ in range(n)] for _ in range(SETS)]
    v = {}
    if c == 4:
        bgra = []
        for im in imgs:
            buf = torch.zeros((h, w * 4 + 256), dtype=torch.uint8, device="cuda")
            q = buf[:, :w * 4].view(h, w, 4)
            q.copy_(im[..., [2, 1, 0, 3]])
            bgra.append(q)
        tmp = [[torch.empty_like(im) for im in imgs] for _ in range(SETS)]
        perm = torch.tensor([2, 1, 0, 3], device="cuda")
        v["a"] = ("submit", lambda k: imgs, None)
        v["b"] = ("submit_ex", lambda k: bgra, "bgra")

        def c_copy(k):
            for src, dst in zip(bgra, tmp[k]):
                torch.index_select(src, 2, perm, out=dst)  # (the gather + contiguous of a permuted view, written straight into place)
            return tmp[k]
        v["c"] = ("submit", c_copy, None)
    else:
        bgr = [im[..., [2, 1, 0]].contiguous() for im in imgs]
        rgbx = []
        for im in imgs:
            q = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
            q[..., :3] = im
            rgbx.append(q[..., :3])
        tmp = [[torch.empty_like(im) for im in imgs] for _ in range(SETS)]
        v["d"] = ("submit", lambda k: imgs, None)
        v["e1"] = ("submit_ex", lambda k: bgr, "bgr")
        v["e2"] = ("submit_ex", lambda k: rgbx, "rgb")

        def f_copy(k):
            for src, dst in zip(rgbx, tmp[k]):
                dst.copy_(src)
            return tmp[k]
        v["f"] = ("submit", f_copy, None)
    return name, w, h, c, n, outs, v


def window(enc, n, outs, var, steps):
    how, src, order = var
    tickets = [None] * SETS
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for s in range(steps):
        k = s % SETS
        if tickets[k] is not None:
            enc.wait(tickets[k], n)  # (this output set's previous submission: done before its buffers are written again)
        ims = src(k)
        if how == "submit":
            enc.submit(ims, outs[k], 0)
        else:
            enc.submit_ex(ims, outs[k], 0, order=order)
        tickets[k] = enc.last_ticket
    enc.join()
    e1.record()
    e1.synchronize()
    enc.finish(n)
    return e0.elapsed_time(e1) / steps


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    enc = fpng_amd.Encoder(device=0)
    for args in (("8 x 8K RGBA grad", 7680, 4320, 4, 8), ("256 x 1080p RGB grad", 1920, 1080, 3, 256)):
        name, w, h, c, n, outs, v = workload(*args)
        ref = None
        for key, var in v.items():  # the files first: every variant writes the packed path's bytes
            window(enc, n, outs, var, 1)
            res = enc.finish(n)  # (the records of the window's one submission)
            got = [(r[0], fpng_amd.fpng_crc32(outs[0][i][:r[0]].cpu().numpy())) for i, r in enumerate(res)]
            ref = ref or got
            assert got == ref, f"{name}: variant {key} wrote other files than the packed path"
        for key, var in v.items():  # warm-up
            window(enc, n, outs, var, 4)
        t = {key: [] for key in v}
        for _ in range(rounds):
            for key, var in v.items():
                t[key].append(window(enc, n, outs, var, steps))
        base = statistics.median(t["a" if c == 4 else "d"])
        print(f"{name}: {rounds} rounds x {steps} steps, median ms per step (min-max), relative to the packed path", flush=True)
        for key in v:
            m = statistics.median(t[key])
            print(f"  {key:3s} {m:8.4f} ms ({min(t[key]):.4f}-{max(t[key]):.4f})  {m / base:6.3f}  {n * w * h / m / 1e6:7.1f} GP/s", flush=True)
        del outs, v
        torch.cuda.empty_cache()
    enc.close()


if __name__ == "__main__":
    main()
