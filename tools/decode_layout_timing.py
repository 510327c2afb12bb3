#!/usr/bin/env python
"""Cost of a destination layout (Encoder.decode_device_ex) against the packed decode and against decoding packed, then repacking,
on the same box in one process.

    python tools/decode_layout_timing.py [rounds] [steps]

Per workload and variant, a window of `steps` back-to-back calls on a descriptor built once (files in device memory; a decode call
returns when its pixels are there), timed on the host clock; the variants take turns round by round and the median window is
reported per call.  Variants:
  8 x 8K RGBA grad:         a  packed RGBA             b  BGRA, pitch w*4 + 256, through _ex     c  a, then a torch gather into BGRA
  256 x 1080p RGB grad:     d  packed RGB              e1 BGR through _ex    e2 RGBX through _ex   f  d, then a torch gather into BGR
                            d4 packed, desired 4 (the bytes e2 writes)
  64 x 1024x768 RGBA stored: g  packed RGBA            h  BGRA through _ex
Every _ex variant's pixels are checked against the packed path's, permuted with torch, first."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fpng_amd  # noqa: E402  (before the first torch.cuda call: the library sets the hardware queue count)
import torch  # noqa: E402


def files(enc, w, h, c, n, flags, distinct=4):
    pngs = []
    for i in range(distinct):
        im = torch.from_numpy(fpng_amd.synth_image("grad", w, h, c, seed=12345 + i)).cuda()
        (p,), _ = enc.encode_tensors([im], flags)
        pngs.append(p)
    return [torch.frombuffer(bytearray(pngs[i % distinct]), dtype=torch.uint8).cuda() for i in range(n)]


def workload(enc, name, w, h, c, n, flags):
    dev = files(enc, w, h, c, n, flags)
    packed = enc.make_decode_batch(dev, c, [(w, h)] * n)
    v = {}
    if c == 4:
        bgra = [torch.zeros((h, w * 4 + 256), dtype=torch.uint8, device="cuda")[:, :w * 4].view(h, w, 4) for _ in range(n)]
        tmp = [torch.empty((h, w, 4), dtype=torch.uint8, device="cuda") for _ in range(n)]
        perm = torch.tensor([2, 1, 0, 3], device="cuda")
        ex = enc.make_decode_batch_ex(dev, bgra, "bgra")
        checks = [(ex, bgra, lambda p: p[..., [2, 1, 0, 3]])]

        def repack():
            enc.decode_device(packed, results=False)
            for src, dst in zip(packed.outs, tmp):
                torch.index_select(src.view(h, w, 4), 2, perm, out=dst)
            torch.cuda.synchronize()
        keys = ("a", "b", "c") if flags != 2 else ("g", "h")
        v[keys[0]] = lambda: enc.decode_device(packed, results=False)
        v[keys[1]] = lambda: enc.decode_device_ex(ex, results=False)
        if flags != 2:
            v[keys[2]] = repack
    else:
        bgr = [torch.empty((h, w, 3), dtype=torch.uint8, device="cuda") for _ in range(n)]
        rgbx = [torch.empty((h, w, 4), dtype=torch.uint8, device="cuda") for _ in range(n)]
        tmp = [torch.empty((h, w, 3), dtype=torch.uint8, device="cuda") for _ in range(n)]
        perm = torch.tensor([2, 1, 0], device="cuda")
        ex1 = enc.make_decode_batch_ex(dev, bgr, "bgr")
        ex2 = enc.make_decode_batch_ex(dev, rgbx, "rgbx")
        checks = [(ex1, bgr, lambda p: p.flip(2)), (ex2, rgbx, lambda p: torch.cat([p, torch.full_like(p[..., :1], 255)], 2))]

        def repack():
            enc.decode_device(packed, results=False)
            for src, dst in zip(packed.outs, tmp):
                torch.index_select(src.view(h, w, 3), 2, perm, out=dst)
            torch.cuda.synchronize()
        v["d"] = lambda: enc.decode_device(packed, results=False)
        v["e1"] = lambda: enc.decode_device_ex(ex1, results=False)
        v["e2"] = lambda: enc.decode_device_ex(ex2, results=False)
        v["f"] = repack
        packed4 = enc.make_decode_batch(dev, 4, [(w, h)] * n)
        v["d4"] = lambda: enc.decode_device(packed4, results=False)
    enc.decode_device(packed, results=False)
    assert all(s == 0 for s in packed.statuses())
    for ex, outs, f in checks:
        enc.decode_device_ex(ex, results=False)
        assert all(s == 0 for s in ex.statuses())
        for p, o in zip(packed.outs, outs):
            assert torch.equal(o, f(p.view(h, w, c))), f"{name}: an _ex variant wrote other pixels than the packed path"
    return v


def window(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    enc = fpng_amd.Encoder(device=0)
    for args in (("8 x 8K RGBA grad", 7680, 4320, 4, 8, 0), ("256 x 1080p RGB grad", 1920, 1080, 3, 256, 0),
                 ("64 x 1024x768 RGBA stored", 1024, 768, 4, 64, 2)):
        name, w, h, c, n, _ = args
        v = workload(enc, *args)
        for fn in v.values():  # warm-up
            window(fn, 3)
        t = {key: [] for key in v}
        for _ in range(rounds):
            for key, fn in v.items():
                t[key].append(window(fn, steps))
        base = statistics.median(next(iter(t.values())))
        print(f"{name}: {rounds} rounds x {steps} calls, median ms per call (min-max), relative to the packed path", flush=True)
        for key in v:
            m = statistics.median(t[key])
            print(f"  {key:3s} {m:8.4f} ms ({min(t[key]):.4f}-{max(t[key]):.4f})  {m / base:6.3f}  {n * w * h / m / 1e6:7.1f} GP/s", flush=True)
        del v
        torch.cuda.empty_cache()
    enc.close()


if __name__ == "__main__":
    main()
