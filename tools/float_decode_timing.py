#!/usr/bin/env python
"""What decoding straight into normalised float CHW tensors costs against what a loader did before it -- decode_device_planar into
uint8 planes, then torch's x.to(dtype) * scale + bias -- on the same box in one process.

    python tools/float_decode_timing.py [rounds] [steps]

The workloads and the device-resident files of tools/planar_timing.py (8 x 8K RGBA grad, 256 x 1080p RGB grad), decode only.  The
variants take turns round by round; a window is `steps` back-to-back calls on descriptors built once, timed on the host clock around
a device synchronise; the median window is reported per call with its min-max.  Variants, per dtype (float32, float16, bfloat16):
  u   decode_device_planar into uint8 NCHW: the yardstick, the path that was there before (once per workload)
  a   u, then nchw.to(dtype) * scale + bias with (1, c, 1, 1) constants of that dtype: three torch kernels and their temporaries
  b   decode_device_float into a preallocated NCHW tensor of that dtype: the fused call
b's values are checked first against a float64 evaluation of the same constants (half an ulp of the dtype).  For b the line also
gives the bytes the call must store over its time: the achieved store bandwidth of the whole call, not of one kernel."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fpng_amd  # noqa: E402  (before the first torch.cuda call: the library sets the hardware queue count)
import torch  # noqa: E402

MEAN, STD = (0.485, 0.456, 0.406, 0.5), (0.229, 0.224, 0.225, 0.25)


def window(fn, m):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(m):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / m


def workload(enc, name, w, h, c, n, rounds, steps):
    pngs = []
    for i in range(4):
        (p,), _ = enc.encode_tensors([torch.from_numpy(fpng_amd.synth_image("grad", w, h, c, seed=12345 + i)).cuda()], 0)
        pngs.append(p)
    dev = [torch.frombuffer(bytearray(pngs[i % 4]), dtype=torch.uint8).cuda() for i in range(n)]
    nchw = torch.empty((n, c, h, w), dtype=torch.uint8, device="cuda")
    planar = enc.make_decode_batch_planar(dev, list(nchw))
    scale, bias = fpng_amd.normalize_constants(MEAN[:c], STD[:c])
    ok = True
    print(f"{name}, decode, {rounds} rounds x {steps} calls: median ms per call (min-max)", flush=True)
    for dtype in (torch.float32, torch.float16, torch.bfloat16):
        out = torch.empty((n, c, h, w), dtype=dtype, device="cuda")
        fused = enc.make_decode_batch_float(dev, list(out), mean=MEAN[:c], std=STD[:c])
        s_t = torch.from_numpy(scale[:c].copy()).cuda().to(dtype).view(1, c, 1, 1)
        b_t = torch.from_numpy(bias[:c].copy()).cuda().to(dtype).view(1, c, 1, 1)
        keep = {}

        def dec_u():
            enc.decode_device_planar(planar, results=False)

        def dec_a():
            enc.decode_device_planar(planar, results=False)
            keep["a"] = nchw.to(dtype) * s_t + b_t

        def dec_b():
            enc.decode_device_float(fused, results=False)
        v = {"u": dec_u, "a": dec_a, "b": dec_b}
        for fn in v.values():
            fn()
        torch.cuda.synchronize()
        assert all(s == 0 for s in planar.statuses()) and all(s == 0 for s in fused.statuses())
        # the fused values: within half an ulp of the dtype (and the float32 constants' rounding) of a float64 evaluation, image by image
        rel = {torch.float32: 2.0 ** -23, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}[dtype]
        s64 = torch.from_numpy(scale[:c].astype("float64")).cuda().view(c, 1, 1)
        b64 = torch.from_numpy(bias[:c].astype("float64")).cuda().view(c, 1, 1)
        for i in range(min(n, 4)):
            want = nchw[i].double() * s64 + b64
            assert bool(((out[i].double() - want).abs() <= 1e-6 + rel * want.abs()).all()), f"{name}: fused {dtype} values are off"
        keep.clear()
        for fn in v.values():
            window(fn, 3)
        t = {key: [] for key in v}
        for _ in range(rounds):
            for key, fn in v.items():
                t[key].append(window(fn, steps))
        keep.clear()
        med = {key: statistics.median(t[key]) for key in t}
        stored = n * c * h * w * out.element_size()
        print(f"  {str(dtype).replace('torch.', ''):9s}", flush=True)
        for key in t:
            extra = f"  {stored / med[key] / 1e6:7.1f} GB/s stored" if key == "b" else ""
            print(f"    {key}  {med[key]:8.4f} ms ({min(t[key]):.4f}-{max(t[key]):.4f})  {n * w * h / med[key] / 1e6:7.1f} GP/s{extra}", flush=True)
        apart = max(t["b"]) < min(t["a"])
        ok &= apart
        print(f"    b / a = {med['b'] / med['a']:.3f}   b / u = {med['b'] / med['u']:.3f}   b < a, ranges apart: {'YES' if apart else 'NO'}", flush=True)
        del out, fused
        torch.cuda.empty_cache()
    return ok


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    enc = fpng_amd.Encoder(device=0)
    ok = True
    for args in (("8 x 8K RGBA grad", 7680, 4320, 4, 8), ("256 x 1080p RGB grad", 1920, 1080, 3, 256)):
        ok &= workload(enc, *args, rounds, steps)
        torch.cuda.empty_cache()
    enc.close()
    print("fused faster than decode + torch for every dtype and workload, ranges apart:", "YES" if ok else "NO")
    return 0


if __name__ == "__main__":
    sys.exit(main())
