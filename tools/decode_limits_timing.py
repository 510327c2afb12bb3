#!/usr/bin/env python
"""Wall time of ONE decode call per destination on the files of tests/test_gpu_decode_limits.py whose dimension is 2^24 -- rows of
2^26 bytes in 65536 column blocks, and 349526 look-back segments in one column -- so that a chain that takes seconds is written
down (profiles/decode_limits.txt) and not discovered later.

    python tools/decode_limits_timing.py

The files are the test's own (the oracle's file with IHDR corrected to the true dimensions), device-resident.  Every call is made
twice on descriptors and outputs built before it and timed on the host clock around a device synchronise: `first` includes the
growth of the encoder's scratch for that file, `again` does not.  One run, no statistics: these are orders of magnitude."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fpng_amd  # noqa: E402  (before the first torch.cuda call: the library sets the hardware queue count)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import container_mutator as CM  # noqa: E402
from cpu_ref import oracle  # noqa: E402
from test_gpu_decode_limits import PATCHED_BIG, smooth_image  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    enc = fpng_amd.Encoder(device=0)
    print(f"box: {torch.cuda.get_device_name(0)}, torch {torch.__version__}; ms per call: first / again", flush=True)
    rng = np.random.default_rng(43)
    warm = torch.frombuffer(bytearray(oracle().encode(smooth_image(64, 97, 4, rng), 64, 97, 4, 0)), dtype=torch.uint8).cuda()
    assert enc.decode_device([warm], 4, [(64, 97)])[0][0] == 0
    for (w, h, c, (fl,)) in PATCHED_BIG:
        img = smooth_image(w, h, c, rng)
        png = CM.with_dimensions(oracle().encode(img, w, h, c, fl), w, h)
        del img
        dev = [torch.frombuffer(bytearray(png), dtype=torch.uint8).cuda()]
        print(f"{w} x {h} x {c}, flags {fl}, {len(png)} bytes", flush=True)
        crops = [(max(w - 5, 0), max(h - 2, 0), min(w, 5), min(h, 2))] + ([(0, h - 50, w, 50)] if h > w else [(w - 300, 0, 300, h), (255, 0, 2, h)])
        calls = []
        for d in (3, 4):
            out = [torch.empty(w * h * d, dtype=torch.uint8, device="cuda")]
            calls.append((f"decode_device, {d} channels", lambda d=d, out=out: enc.decode_device(dev, d, [(w, h)], out)))
        ex = torch.empty((h, w, 4), dtype=torch.uint8, device="cuda")
        calls.append(("decode_device_ex, bottom-up BGRA", lambda: enc.decode_device_ex(dev, [ex], order="bgra", bottom_up=True)))
        pl = torch.empty((c, h, w), dtype=torch.uint8, device="cuda")
        calls.append(("decode_device_planar", lambda: enc.decode_device_planar(dev, [pl])))
        fo = torch.empty((c, h, w), dtype=torch.float16, device="cuda")
        calls.append(("decode_device_float, f16", lambda: enc.decode_device_float(dev, [fo], scale=[1.0 / 255.0] * 4, bias=[0.0] * 4)))
        for dt in (torch.uint8, torch.bfloat16):
            for crop in crops:
                co = torch.empty((3, crop[3], crop[2]), dtype=dt, device="cuda")
                kw = {} if dt == torch.uint8 else {"scale": [1.0 / 255.0] * 4, "bias": [0.0] * 4}
                calls.append((f"decode_device_crop {crop}, {str(dt)[6:]}", lambda crop=crop, co=co, kw=kw: enc.decode_device_crop(dev, [crop], [co], **kw)))

        def verified():
            enc.set_decode_verify(3)
            try:
                return enc.decode_device(dev, 4, [(w, h)], out)
            finally:
                enc.set_decode_verify(0)
        calls.append(("decode_device, 4 channels, CRC-32 and Adler-32 verified", verified))
        if c == 4:
            calls.append(("decode_host, 4 channels (streamed; with the download)", lambda: [enc.decode_host(png, 4)]))
        for name, fn in calls:
            first, got = timed(fn)
            again, got = timed(fn)
            print(f"  {name:62s} {first:10.2f} / {again:10.2f}   status {got[0][0]}", flush=True)
        del dev, ex, pl, fo, out
        torch.cuda.empty_cache()
    enc.close()


if __name__ == "__main__":
    main()
