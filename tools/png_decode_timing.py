#!/usr/bin/env python
"""The general decode tier on ordinary PNG files (Encoder.decode_device_png) next to Pillow on the CPU.

    python tools/png_decode_timing.py [regions=5] [calls per region=3] [cpu threads=16] [> profiles/<name>.txt]

Two batches of files that Pillow writes at compress_level 6: 256 x 512x512 RGB and 8 x 3840x2160 RGBA.  The GPU figure is the
median over `regions` timed regions (device events around `calls` calls each, after a warm-up call) of one call of the whole batch,
files in device memory; the kernels' share comes from a further call with profiling on (events around the two kernels).  Pillow
decodes the same files from memory with `cpu threads` threads (its decoder releases the interpreter lock), median of the same number
of regions.  The pixels are compared once."""
import io
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from PIL import Image

import fpng_amd

regions = int(sys.argv[1]) if len(sys.argv) > 1 else 5
calls = int(sys.argv[2]) if len(sys.argv) > 2 else 3
threads = int(sys.argv[3]) if len(sys.argv) > 3 else 16


def picture(w, h, c, seed):
    """smooth ramps with some noise on them, a different picture per seed"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([(x * (k + 1 + seed % 3) // 4 + y * (3 - k) // 2 + 40 * seed) & 255 for k in range(c)], axis=-1)
    return ((base + rng.integers(0, 12, (h, w, c))) & 255).astype(np.uint8)


def pillow_file(img):
    buf = io.BytesIO()
    Image.fromarray(img, "RGB" if img.shape[2] == 3 else "RGBA").save(buf, "PNG", compress_level=6)
    return buf.getvalue()


def pillow_decode(f):
    with Image.open(io.BytesIO(f)) as im:
        im.load()
        return im


assert torch.cuda.is_available(), "this measurement needs the GPU"
enc = fpng_amd.Encoder(device=0)
print(f"device: {torch.cuda.get_device_name(0)}; {regions} regions of {calls} calls; Pillow {Image.__version__} on {threads} threads")
for name, w, h, c, n in (("256 x 512x512 RGB", 512, 512, 3, 256), ("8 x 3840x2160 RGBA", 3840, 2160, 4, 8)):
    imgs = [picture(w, h, c, i) for i in range(n)]
    files = [pillow_file(im) for im in imgs]
    dev = [torch.frombuffer(bytearray(f), dtype=torch.uint8).cuda() for f in files]
    outs = [torch.empty(w * h * c, dtype=torch.uint8, device="cuda") for _ in range(n)]
    batch = enc.make_decode_batch_png(dev, c, outs=outs)
    enc.decode_device_png(batch, results=False)  # warm-up; the pixels are checked once
    for (st, px, _), im in zip(batch.results(), imgs):
        assert st == 0 and np.array_equal(px.cpu().numpy(), im)
    ms = []
    for _ in range(regions):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(calls):
            enc.decode_device_png(batch, results=False)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / calls)
    gpu = statistics.median(ms)
    enc.set_profiling(True)
    enc.decode_device_png(batch, results=False)
    k_inf, k_unf = enc.last_decode_png_kernel_ms()
    enc.set_profiling(False)
    with ThreadPoolExecutor(threads) as pool:
        list(pool.map(pillow_decode, files))  # warm-up
        cpu = []
        for _ in range(regions):
            t0 = time.perf_counter()
            list(pool.map(pillow_decode, files))
            cpu.append((time.perf_counter() - t0) * 1e3)
    cpu = statistics.median(cpu)
    mb, mpx = sum(len(f) for f in files) / 1e6, n * w * h / 1e6
    print(f"{name}: {mb:.1f} MB of PNG -> {mpx * c:.0f} MB of pixels")
    print(f"  decode_device_png   {gpu:9.3f} ms per call (min {min(ms):.3f}, max {max(ms):.3f}) = {mpx / gpu:8.2f} GP/s")
    print(f"    png_inflate_kernel  {k_inf:9.3f} ms, png_unfilter_kernel {k_unf:9.3f} ms: {100 * (k_inf + k_unf) / gpu:.0f} % of the call in the kernels")
    print(f"  Pillow, {threads} threads  {cpu:9.3f} ms per batch = {mpx / cpu:8.2f} GP/s", flush=True)
enc.close()
