#!/usr/bin/env python
"""What decoding several views of each file into CHANNELS-LAST batches costs through fpng_amd_decode_batch_device_hwc_views, against
the way there was before it -- the planar views call into NCHW batches followed by x.contiguous(memory_format=torch.channels_last)
-- and against the planar call alone, the floor the interleaved store is held against; one box, one process (a sibling of
tools/views_timing.py, whose workloads, files, window, rounds and steps it uses).

    python tools/views_hwc_timing.py time   [rounds] [steps] [files]
    python tools/views_hwc_timing.py kernel <a|b> <hwc|planar+copy|planar> [calls] [files]

256 device-resident 1080p RGB files, f16 with ImageNet's mean / std, every second view mirrored; workloads a and b of views_timing.py.
One batch per view size: (files x views of that size, 3, side, side), channels_last on the hwc side (file i's view j is
x[...].permute(1, 2, 0)), NCHW on the other two.
time    The three sides take turns round by round; a window is `steps` back-to-back calls between two device events, after a warm-up
        of all; the median window per call with its min-max over the rounds.  Before timing, hwc and planar+copy are compared:
        bit for bit the same batches.
kernel  `calls` calls of one side of one workload and nothing else: run it under `rocprofv3 --kernel-trace --stats` and read the
        resize kernels' (and, for planar+copy, the copy kernel's) time per call from the statistics."""
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
from views_timing import WORKLOADS, random_resized_crop, spread  # noqa: E402

SIDES = ("hwc", "planar+copy", "planar")


class Sides:
    """the descriptors of one workload: the same crops, views and constants; a batch per view size and side"""

    def __init__(self, enc, dev, key, which=SIDES):
        n, spec = len(dev), WORKLOADS[key]
        rng = np.random.default_rng(2024)
        self.enc, self.key, self.n, self.v = enc, key, n, len(spec)
        crops = [[random_resized_crop(rng, scale) for _, scale in spec] for _ in range(n)]
        fulls = [[(side, side) for side, _ in spec] for _ in range(n)]
        mirrors = [[bool(k & 1) for k in range(len(spec))] for _ in range(n)]
        per_size = {side: sum(s == side for s, _ in spec) for side, _ in spec}
        slot, seen = [], {}
        for side, _ in spec:  # view k of a file is image number slot[k] of its size among the file's
            slot.append(seen.get(side, 0))
            seen[side] = slot[-1] + 1
        self.batches, self.db, self.copied = {}, {}, {}
        for name in which:
            hwc = name == "hwc"
            x = {side: torch.empty((n * cnt, 3, side, side), dtype=torch.float16, device="cuda", memory_format=torch.channels_last if hwc else torch.contiguous_format)
                 for side, cnt in per_size.items()}
            outs = [[x[side][i * per_size[side] + slot[k]] for k, (side, _) in enumerate(spec)] for i in range(n)]
            if hwc:
                self.db[name] = enc.make_decode_batch_views_hwc(dev, crops, [[t.permute(1, 2, 0) for t in ts] for ts in outs], fulls, mirror=mirrors, mean=MEAN, std=STD)
            else:
                self.db[name] = enc.make_decode_batch_views(dev, crops, outs, fulls, mirror=mirrors, mean=MEAN, std=STD)
            self.batches[name] = x

    def run(self, name):
        if name == "hwc":
            self.enc.decode_device_views_hwc(self.db[name], results=False)
        else:
            self.enc.decode_device_views(self.db[name], results=False)
            if name == "planar+copy":  # (the parent's way to a channels-last batch: a permute copy of every batch, on the same stream)
                self.copied = {side: x.contiguous(memory_format=torch.channels_last) for side, x in self.batches[name].items()}

    def check(self):
        for name in self.db:
            self.run(name)
        torch.cuda.synchronize()
        assert all(s == 0 for d in self.db.values() for s in d.statuses())
        if "hwc" in self.db and "planar+copy" in self.db:
            for side, x in self.batches["hwc"].items():
                y = self.copied[side]
                assert x.is_contiguous(memory_format=torch.channels_last) and y.is_contiguous(memory_format=torch.channels_last) and x.stride() == y.stride()
                assert torch.equal(x.view(torch.int16), y.view(torch.int16)), "the hwc call's batch is not the planar call's, copied to channels_last"
            return True
        return False


def overlap(a, b):
    return "do not overlap" if max(a) < min(b) or max(b) < min(a) else "OVERLAP"


def time_mode(rounds, steps, n):
    enc = fpng_amd.Encoder(device=0)
    dev = files_on_device(enc, W, H, n)
    for key in WORKLOADS:
        s = Sides(enc, dev, key)
        assert s.check()
        print(f"workload {key}: {n} x 1080p RGB, {s.v} views per file -> f16; hwc and planar+copy hold bit-identical channels-last batches", flush=True)
        for name in s.db:
            window(lambda: s.run(name), 3)
        t = {name: [] for name in s.db}
        for _ in range(rounds):
            for name in s.db:
                t[name].append(window(lambda: s.run(name), steps))
        for name in t:
            print(f"    {name:11s} {spread(t[name])} per call, {rounds} rounds x {steps} calls", flush=True)
        m = {name: statistics.median(t[name]) for name in t}
        print(f"    hwc / planar+copy = {m['hwc'] / m['planar+copy']:.3f}; the gap {m['planar+copy'] - m['hwc']:+.4f} ms; ranges {overlap(t['hwc'], t['planar+copy'])}", flush=True)
        print(f"    hwc / planar      = {m['hwc'] / m['planar']:.3f}; the gap {m['hwc'] - m['planar']:+.4f} ms against planar's own range {max(t['planar']) - min(t['planar']):.4f} ms; "
              f"ranges {overlap(t['hwc'], t['planar'])}", flush=True)
        del s
    enc.close()


def kernel_mode(key, name, calls, n):
    enc = fpng_amd.Encoder(device=0)
    s = Sides(enc, files_on_device(enc, W, H, n), key, which=(name,))
    s.check()
    for _ in range(calls):
        s.run(name)
    torch.cuda.synchronize()
    print(f"workload {key}, {name}: {calls} calls after one, {n} files x {s.v} views", flush=True)
    enc.close()


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    nums = [int(a) for a in sys.argv[2:] if a.isdigit()]
    if mode == "kernel" and len(sys.argv) >= 4 and sys.argv[2] in WORKLOADS and sys.argv[3] in SIDES:
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
