#!/usr/bin/env python
"""The un-filter kernels of the general decode tier on tools/png_decode_timing.py's 256 x 512x512 RGB batch (Pillow, level 6).

    python tools/png_views_timing.py [regions=5] [calls per region=3] [png: the existing call alone] [> profiles/<name>.txt]

decode_device_png: the call's time per region (device events around `calls` calls, after a warm-up call) and, from one further call
per region with profiling on, png_unfilter_kernel's.  decode_device_png_views (where the library has it; every file through the
general tier, uint8 planar destinations, one identity view per file): png_unfilter_box_kernel's time, the same way, for the whole
image as box and for a 224 x 224 box in the image's top-left and in its bottom-right quarter.  Every figure: median (min, max) over
the regions.  The pixels of each form are compared once."""
import io
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from PIL import Image

import fpng_amd

regions = int(sys.argv[1]) if len(sys.argv) > 1 else 5
calls = int(sys.argv[2]) if len(sys.argv) > 2 else 3
W = H = 512
N = 256


def picture(w, h, c, seed):
    """(tools/png_decode_timing.py's)"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([(x * (k + 1 + seed % 3) // 4 + y * (3 - k) // 2 + 40 * seed) & 255 for k in range(c)], axis=-1)
    return ((base + rng.integers(0, 12, (h, w, c))) & 255).astype(np.uint8)


def fmt(v):
    return f"{statistics.median(v):9.3f} ms (min {min(v):.3f}, max {max(v):.3f})"


def timed(run):
    """-> (per call ms per region, the two kernels' ms per region)"""
    run()
    per_call, k0, k1 = [], [], []
    for _ in range(regions):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(calls):
            run()
        e1.record()
        torch.cuda.synchronize()
        per_call.append(e0.elapsed_time(e1) / calls)
        enc.set_profiling(True)
        run()
        a, b = enc.last_decode_png_kernel_ms()
        enc.set_profiling(False)
        k0.append(a), k1.append(b)
    return per_call, k0, k1


assert torch.cuda.is_available(), "this measurement needs the GPU"
enc = fpng_amd.Encoder(device=0)
print(f"device: {torch.cuda.get_device_name(0)}; {regions} regions of {calls} calls; {N} x {W}x{H} RGB, Pillow {Image.__version__}, compress_level 6")
imgs = [picture(W, H, 3, i) for i in range(N)]
files = []
for im in imgs:
    buf = io.BytesIO()
    Image.fromarray(im, "RGB").save(buf, "PNG", compress_level=6)
    files.append(buf.getvalue())
dev = [torch.frombuffer(bytearray(f), dtype=torch.uint8).cuda() for f in files]
outs = [torch.empty(W * H * 3, dtype=torch.uint8, device="cuda") for _ in range(N)]
batch = enc.make_decode_batch_png(dev, 3, outs=outs)
per_call, k_inf, k_unf = timed(lambda: enc.decode_device_png(batch, results=False))
for (st, px, _), im in zip(batch.results(), imgs):
    assert st == 0 and np.array_equal(px.cpu().numpy(), im)
print(f"decode_device_png          per call {fmt(per_call)}")
print(f"  png_inflate_kernel                {fmt(k_inf)}")
print(f"  png_unfilter_kernel               {fmt(k_unf)}", flush=True)
if hasattr(enc, "decode_device_png_views") and sys.argv[3:4] != ["png"]:
    for name, (x, y, w, h) in (("the whole image", (0, 0, W, H)), ("224 x 224 at (0, 0)", (0, 0, 224, 224)), ("224 x 224 at (288, 288)", (288, 288, 224, 224))):
        vouts = [[torch.empty((3, h, w), dtype=torch.uint8, device="cuda")] for _ in range(N)]
        vb = enc.make_decode_batch_png_views(dev, [[(x, y, w, h)]] * N, vouts, (w, h), flags=fpng_amd.FPNG_AMD_PNG_GENERAL_ONLY)
        per_call, k_inf, k_box = timed(lambda: enc.decode_device_png_views(vb, results=False))
        for (st, _, _), (t,), im in list(zip(vb.results(), vouts, imgs))[::37]:
            assert st == 0 and np.array_equal(t.cpu().numpy().transpose(1, 2, 0), im[y:y + h, x:x + w])
        print(f"decode_device_png_views, box {name}: per call {fmt(per_call)}")
        print(f"  png_inflate_kernel                {fmt(k_inf)}")
        print(f"  png_unfilter_box_kernel           {fmt(k_box)}", flush=True)
enc.close()
