#!/usr/bin/env python
"""What encoding straight from float CHW tensors costs against what a caller did before it -- torch's
x.mul(scale).add(bias).round().clamp(0, 255).to(torch.uint8), then submit_planar -- on the same box in one process.

    python tools/float_encode_timing.py [rounds] [steps]

8 x 8K RGBA grad and 64 x 1080p RGB grad, device-resident, flags 0.  The floats are (byte / 255 - mean) / std of the synthetic
bytes in each dtype, so that every variant writes the same files.  The variants take turns round by round; a window is `steps`
back-to-back calls on descriptors built once, timed on the host clock around a device synchronise; the median window is reported
per call with its min-max.  Variants, per dtype (float32, float16, bfloat16):
  a   submit_float on the float NCHW tensor: the fused call
  b   the torch chain above into a fresh uint8 NCHW tensor, then submit_planar on it: the yardstick, the path that was there before
  c   submit_planar alone on planes quantised beforehand: what the walk costs without any conversion
a's files are checked first against b's, byte for byte.  For a the line also gives the source bytes the call must read over its
time: the achieved load bandwidth of the whole call, not of one kernel."""
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
    nchw8 = torch.empty((n, c, h, w), dtype=torch.uint8, device="cuda")
    for i in range(n):
        nchw8[i].copy_(torch.from_numpy(fpng_amd.synth_image("grad", w, h, c, seed=12345 + i % 4)).cuda().permute(2, 0, 1))
    cap = fpng_amd.max_encoded_size(w, h, c) + 64
    outs = {k: [torch.empty(cap, dtype=torch.uint8, device="cuda") for _ in range(n)] for k in "abc"}
    scale, bias = fpng_amd.denormalize_constants(MEAN[:c], STD[:c])
    planar_c = enc.make_batch_planar(list(nchw8), outs["c"])
    m_t = torch.tensor(MEAN[:c], dtype=torch.float32, device="cuda").view(1, c, 1, 1)
    s_t = torch.tensor(STD[:c], dtype=torch.float32, device="cuda").view(1, c, 1, 1)
    ok = True
    print(f"{name}, encode, flags 0, {rounds} rounds x {steps} calls: median ms per call (min-max)", flush=True)
    for dtype in (torch.float32, torch.float16, torch.bfloat16):
        x = torch.empty((n, c, h, w), dtype=dtype, device="cuda")
        for i in range(n):  # (image by image: the float32 temporaries of one image, not of the batch)
            x[i].copy_(((nchw8[i:i + 1].to(torch.float32) / 255.0 - m_t) / s_t)[0])
        fused = enc.make_batch_float(list(x), outs["a"], mean=MEAN[:c], std=STD[:c])
        sc_t = torch.from_numpy(scale[:c].copy()).cuda().to(dtype).view(1, c, 1, 1)
        bi_t = torch.from_numpy(bias[:c].copy()).cuda().to(dtype).view(1, c, 1, 1)
        keep = {}

        def enc_a():
            enc.submit_float(fused)

        def enc_b():
            keep["q"] = x.mul(sc_t).add(bi_t).round().clamp(0, 255).to(torch.uint8)
            enc.submit_planar(list(keep["q"]), outs["b"], 0)

        def enc_c():
            enc.submit_planar(planar_c)
        v = {"a": enc_a, "b": enc_b, "c": enc_c}
        sizes = {}
        for key, fn in v.items():
            fn()
            res = enc.wait(enc.last_ticket, n)
            assert all(st == 0 for _, _, st in res)
            sizes[key] = [s for s, _, _ in res]
        # the fused call's files against the torch chain's (bf16's products round before torch's add does, so there the chain itself
        # may be a byte off: reported, not asserted)
        same = sum(sizes["a"][i] == sizes["b"][i] and torch.equal(outs["a"][i][:sizes["a"][i]], outs["b"][i][:sizes["b"][i]]) for i in range(n))
        print(f"  {str(dtype).replace('torch.', ''):9s}  files identical to the torch chain's: {same} of {n}", flush=True)
        if dtype == torch.float32:
            assert same == n, f"{name}: the fused float32 files differ from the torch chain's"
        for fn in v.values():
            window(fn, 3)
        t = {key: [] for key in v}
        for _ in range(rounds):
            for key, fn in v.items():
                t[key].append(window(fn, steps))
        keep.clear()
        med = {key: statistics.median(t[key]) for key in t}
        loaded = n * c * h * w * x.element_size()
        for key in t:
            extra = f"  {loaded / med[key] / 1e6:7.1f} GB/s of source read" if key == "a" else ""
            print(f"    {key}  {med[key]:8.4f} ms ({min(t[key]):.4f}-{max(t[key]):.4f})  {n * w * h / med[key] / 1e6:7.1f} GP/s{extra}", flush=True)
        apart = max(t["a"]) < min(t["b"])
        ok &= apart
        print(f"    a / b = {med['a'] / med['b']:.3f}   a / c = {med['a'] / med['c']:.3f}   a < b, ranges apart: {'YES' if apart else 'NO'}", flush=True)
        enc.finish(n)
        del x, fused
        torch.cuda.empty_cache()
    return ok


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    enc = fpng_amd.Encoder(device=0)
    ok = True
    for args in (("8 x 8K RGBA grad", 7680, 4320, 4, 8), ("64 x 1080p RGB grad", 1920, 1080, 3, 64)):
        ok &= workload(enc, *args, rounds, steps)
        torch.cuda.empty_cache()
    enc.close()
    print("fused faster than the torch chain + submit_planar for every dtype and workload, ranges apart:", "YES" if ok else "NO")
    return 0


if __name__ == "__main__":
    sys.exit(main())
