#!/usr/bin/env python
"""What several views of each file cost through fpng_amd_decode_batch_device_planar_views (one decode per file) against the way
there was before it -- decode_device_resize_view in ONE call with each file listed once per view, the same crops, views and
destinations -- on one box in one process (a sibling of tools/resize_view_timing.py, whose window and rounds it uses).

    python tools/views_timing.py time   [rounds] [steps] [files]
    python tools/views_timing.py kernel <a|b> <views|listed> [calls] [files]

256 device-resident 1080p RGB files (four distinct `grad` images, repeated), f16 with ImageNet's mean / std, every second view mirrored:
  a   two 224 x 224 RandomResizedCrop views per file (area 0.08 ... 1, aspect 3/4 ... 4/3): SimCLR, BYOL, MoCo
  b   two 224 x 224 global views (area 0.4 ... 1) and six 96 x 96 local ones (area 0.05 ... 0.4) per file: DINO / SwAV multi-crop
time    The two sides take turns round by round; a window is `steps` back-to-back calls between two device events, after a warm-up
        of both; the median window per call with its min-max over the rounds, then the phase split of last_decode_phase_ms
        (set_profiling: the first group's kernels; "unfilter" brackets everything behind the synchronisation, the resize included).
        The two sides' batches are compared first: bit for bit the same.
kernel  `calls` calls of one side of one workload and nothing else: run it under `rocprofv3 --kernel-trace --stats` and read the
        resize kernels' time per call from the statistics (the listed side runs the same tiles on the rectangular grid of the
        largest record, the views side on the exact grid: their kernel times are that comparison)."""
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fpng_amd  # noqa: E402  (before the first torch.cuda call: the library sets the hardware queue count)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from resize_decode_timing import H, MEAN, STD, W, window  # noqa: E402
from resize_view_timing import files_on_device  # noqa: E402

WORKLOADS = {"a": [(224, (0.08, 1.0))] * 2, "b": [(224, (0.4, 1.0))] * 2 + [(96, (0.05, 0.4))] * 6}  # per view: (side, area range)


def random_resized_crop(rng, scale):
    """torchvision's RandomResizedCrop.get_params for an area range: ten tries, then the central crop"""
    for _ in range(10):
        area = W * H * rng.uniform(*scale)
        ratio = math.exp(rng.uniform(math.log(3 / 4), math.log(4 / 3)))
        cw, ch = int(round(math.sqrt(area * ratio))), int(round(math.sqrt(area / ratio)))
        if 0 < cw <= W and 0 < ch <= H:
            return int(rng.integers(0, W - cw + 1)), int(rng.integers(0, H - ch + 1)), cw, ch
    return (W - H) // 2, 0, H, H


class Sides:
    """the two descriptors of one workload: the same crops, views and constants, destinations of the same shapes"""

    def __init__(self, enc, dev, key, which=("views", "listed")):
        n, spec = len(dev), WORKLOADS[key]
        rng = np.random.default_rng(2024)
        self.enc, self.key, self.n, self.v = enc, key, n, len(spec)
        crops = [[random_resized_crop(rng, scale) for _, scale in spec] for _ in range(n)]
        fulls = [[(side, side) for side, _ in spec] for _ in range(n)]
        mirrors = [[bool(k & 1) for k in range(len(spec))] for _ in range(n)]
        boxes = [fpng_amd.views_source(c, f) for c, f in zip(crops, fulls)]
        self.box_share = sum(b[2] * b[3] for b in boxes) / (n * W * H)
        self.view_share = sum(fpng_amd.resize_view_source(c, f)[2] * fpng_amd.resize_view_source(c, f)[3] for cs, fs in zip(crops, fulls) for c, f in zip(cs, fs)) / (n * W * H)
        self.outs, self.db = {}, {}
        for side in which:
            self.outs[side] = [[torch.empty((3, s, s), dtype=torch.float16, device="cuda") for s, _ in spec] for _ in range(n)]
        if "views" in which:
            self.db["views"] = enc.make_decode_batch_views(dev, crops, self.outs["views"], fulls, mirror=mirrors, mean=MEAN, std=STD)
        if "listed" in which:  # (file 0's views first: the order of the views call's records)
            flat = lambda nested: [v for per in nested for v in per]  # noqa: E731
            self.db["listed"] = enc.make_decode_batch_resize_view([d for d in dev for _ in spec], flat(crops), flat(self.outs["listed"]), flat(fulls), mirror=flat(mirrors),
                                                                  mean=MEAN, std=STD)

    def run(self, side):
        if side == "views":
            self.enc.decode_device_views(self.db["views"], results=False)
        else:
            self.enc.decode_device_resize_view(self.db["listed"], results=False)

    def check(self):
        for side in self.db:
            self.run(side)
        torch.cuda.synchronize()
        assert all(s == 0 for d in self.db.values() for s in d.statuses())
        if len(self.db) == 2:
            for a, b in zip((t for ts in self.outs["views"] for t in ts), (t for ts in self.outs["listed"] for t in ts)):
                assert torch.equal(a.view(torch.int16), b.view(torch.int16)), "the views call's batch is not the listed call's"


def spread(t):
    return f"{statistics.median(t):8.4f} ms ({min(t):.4f}-{max(t):.4f}, spread {100 * (max(t) - min(t)) / statistics.median(t):.1f} %)"


def time_mode(rounds, steps, n):
    enc = fpng_amd.Encoder(device=0)
    dev = files_on_device(enc, W, H, n)
    for key in WORKLOADS:
        s = Sides(enc, dev, key)
        s.check()
        print(f"workload {key}: {n} x 1080p RGB, {s.v} views per file -> f16; the two sides' batches are bit for bit the same.  Decoded per file: the views' "
              f"bounding box {100 * s.box_share:.0f} % of the image (views call), the sum of the views' own boxes {100 * s.view_share:.0f} % (listed)", flush=True)
        for side in s.db:
            window(lambda: s.run(side), 3)
        t = {side: [] for side in s.db}
        for _ in range(rounds):
            for side in s.db:
                t[side].append(window(lambda: s.run(side), steps))
        for side in t:
            print(f"    {side:7s} {spread(t[side])} per call, {rounds} rounds x {steps} calls", flush=True)
        mv, ml = statistics.median(t["views"]), statistics.median(t["listed"])
        print(f"    views / listed = {mv / ml:.3f}; the gap {ml - mv:+.4f} ms against the two ranges {max(t['views']) - min(t['views']):.4f} and {max(t['listed']) - min(t['listed']):.4f} ms; "
              f"ranges {'do not overlap' if max(t['views']) < min(t['listed']) or max(t['listed']) < min(t['views']) else 'OVERLAP'}", flush=True)
        enc.set_profiling(True)
        ph = {side: [] for side in s.db}
        for _ in range(rounds):
            for side in s.db:
                s.run(side)
                torch.cuda.synchronize()
                ph[side].append(enc.last_decode_phase_ms())
        enc.set_profiling(False)
        for side in ph:
            print(f"    phases, {side:7s} " + "  ".join(f"{name} {statistics.median(p[name] for p in ph[side]):.4f}" for name in ("sync", "offsets", "emit", "unfilter")) + " ms", flush=True)
        del s
    enc.close()


def kernel_mode(key, side, calls, n):
    enc = fpng_amd.Encoder(device=0)
    s = Sides(enc, files_on_device(enc, W, H, n), key, which=(side,))
    s.check()
    for _ in range(calls):
        s.run(side)
    torch.cuda.synchronize()
    print(f"workload {key}, {side}: {calls} calls after one, {n} files x {s.v} views", flush=True)
    enc.close()


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    nums = [int(a) for a in sys.argv[2:] if a.isdigit()]
    if mode == "kernel" and len(sys.argv) >= 4 and sys.argv[2] in WORKLOADS and sys.argv[3] in ("views", "listed"):
        calls, n = (nums + [10, 256][len(nums):])[:2]
    elif mode == "time":
        rounds, steps, n = (nums + [9, 10, 256][len(nums):])[:3]
    else:
        print(__doc__)
        return 2
    assert torch.cuda.is_available(), "this tool measures on a GPU"
    print(f"{torch.cuda.get_device_name(0)}, torch {torch.__version__}, hip {torch.version.hip}", flush=True)
    if mode == "time":
        time_mode(rounds, steps, n)
    else:
        kernel_mode(sys.argv[2], sys.argv[3], calls, n)
    return 0


if __name__ == "__main__":
    sys.exit(main())
