#!/usr/bin/env python
"""What a per-view colour matrix costs inside the views call (fpng_amd_decode_batch_device_planar_views_color / _hwc_views_color)
against what a user does without it -- the plain views call to uint8 batches, then torch for the per-sample matrix, the clamp, the
normalisation and the cast -- and against the plain float views call with no colour at all, the floor; one box, one process (a
sibling of tools/views_hwc_timing.py, whose workloads, files, window, rounds and steps it uses).

    python tools/views_color_timing.py time   [rounds] [steps] [files]
    python tools/views_color_timing.py kernel <a|b> <color|color_hwc|torch|plain> [calls] [files]

256 device-resident 1080p RGB files, f16 with ImageNet's mean / std, every second view mirrored; workloads a and b of views_timing.py;
every view its own color_matrix() of ColorJitter(0.4, 0.4, 0.4, 0.1)-style factors, one view in five grayscale.  One batch per view
size: (files x views of that size, 3, side, side), NCHW but for color_hwc (channels_last; file i's view j is x[...].permute(1, 2, 0)).
  color      the colour call, planar destinations
  color_hwc  the colour call, channels-last destinations
  torch      decode_device_views to uint8 batches, then per batch: baddbmm of the (N, 3, 3) matrices and (N, 3, 1) constants over the
             floats of the bytes, clamp(0, 255), the normalisation's multiply and add, the cast to f16 -- a second batch buffer and
             five elementwise passes (convert, mix, clamp, normalise, cast)
  plain      decode_device_views to f16 with no colour: the floor
time    The sides take turns round by round; a window is `steps` back-to-back calls between two device events, after a warm-up of
        all; the median window per call with its min-max over the rounds, then the share of the stage behind the synchronisation
        (last_decode_phase_ms under set_profiling: "unfilter" brackets the pixel pass and the resize).  Before timing, color and
        color_hwc are compared bit for bit, and torch against color to within the last place of f16: torch's matrix product sums
        in another order and rounds the normalisation in two steps.
kernel  `calls` calls of one side of one workload and nothing else: run it under `rocprofv3 --kernel-trace --stats`."""
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

SIDES = ("color", "color_hwc", "torch", "plain")


def jitter(rng):
    return fpng_amd.color_matrix(brightness=rng.uniform(0.6, 1.4), contrast=rng.uniform(0.6, 1.4), saturation=0.0 if rng.random() < 0.2 else rng.uniform(0.6, 1.4),
                                 hue=rng.uniform(-0.1, 0.1))


class Sides:
    """the descriptors of one workload: the same crops, views, matrices and constants; a batch per view size and side"""

    def __init__(self, enc, dev, key, which=SIDES):
        n, spec = len(dev), WORKLOADS[key]
        rng = np.random.default_rng(2024)
        self.enc, self.key, self.n, self.v = enc, key, n, len(spec)
        crops = [[random_resized_crop(rng, scale) for _, scale in spec] for _ in range(n)]
        fulls = [[(side, side) for side, _ in spec] for _ in range(n)]
        mirrors = [[bool(k & 1) for k in range(len(spec))] for _ in range(n)]
        colors = [[jitter(rng) for _ in spec] for _ in range(n)]
        per_size = {side: sum(s == side for s, _ in spec) for side, _ in spec}
        slot, seen = [], {}
        for side, _ in spec:  # view k of a file is image number slot[k] of its size among the file's
            slot.append(seen.get(side, 0))
            seen[side] = slot[-1] + 1
        self.batches, self.db, self.mixed = {}, {}, {}
        for name in which:
            hwc, u8 = name == "color_hwc", name == "torch"
            x = {side: torch.empty((n * cnt, 3, side, side), dtype=torch.uint8 if u8 else torch.float16, device="cuda",
                                   memory_format=torch.channels_last if hwc else torch.contiguous_format) for side, cnt in per_size.items()}
            outs = [[x[side][i * per_size[side] + slot[k]] for k, (side, _) in enumerate(spec)] for i in range(n)]
            kw = {} if u8 else {"mean": MEAN, "std": STD}
            if name.startswith("color"):
                kw["color"] = colors
            if hwc:
                self.db[name] = enc.make_decode_batch_views_hwc(dev, crops, [[t.permute(1, 2, 0) for t in ts] for ts in outs], fulls, mirror=mirrors, **kw)
            else:
                self.db[name] = enc.make_decode_batch_views(dev, crops, outs, fulls, mirror=mirrors, **kw)
            self.batches[name] = x
        # the torch side's constants: per batch the images' matrices in the batch's order, the normalisation per channel
        self.m, self.k = {}, {}
        for side, cnt in per_size.items():
            ms = np.zeros((n * cnt, 3, 4), dtype=np.float32)
            for i in range(n):
                for k, (s, _) in enumerate(spec):
                    if s == side:
                        ms[i * cnt + slot[k]] = colors[i][k]
            self.m[side] = torch.from_numpy(ms[:, :, :3].copy()).cuda()
            self.k[side] = torch.from_numpy(ms[:, :, 3:].copy()).cuda()
        scale, bias = fpng_amd.normalize_constants(MEAN, STD)
        self.scale = torch.tensor([float(v) for v in scale[:3]], dtype=torch.float32, device="cuda").view(1, 3, 1)
        self.bias = torch.tensor([float(v) for v in bias[:3]], dtype=torch.float32, device="cuda").view(1, 3, 1)

    def run(self, name):
        if name == "color_hwc":
            self.enc.decode_device_views_hwc(self.db[name], results=False)
            return
        self.enc.decode_device_views(self.db[name], results=False)
        if name == "torch":  # (what the colour call replaces: on the same stream, behind the decode)
            for side, x in self.batches[name].items():
                f = x.view(x.shape[0], 3, -1).float()                        # convert
                y = torch.baddbmm(self.k[side], self.m[side], f)             # mix: the per-sample matrix and constant
                y.clamp_(0.0, 255.0)                                         # clamp
                y.mul_(self.scale).add_(self.bias)                           # normalise
                self.mixed[side] = y.to(torch.float16).view(x.shape)         # cast

    def check(self):
        for name in self.db:
            self.run(name)
        torch.cuda.synchronize()
        assert all(s == 0 for d in self.db.values() for s in d.statuses())
        notes = []
        if "color" in self.db and "color_hwc" in self.db:
            for side, x in self.batches["color"].items():
                y = self.batches["color_hwc"][side]
                assert y.is_contiguous(memory_format=torch.channels_last)
                assert torch.equal(x.view(torch.int16), y.contiguous().view(torch.int16)), "the two layouts of the colour call differ"
            notes.append("color and color_hwc hold bit-identical elements")
        if "color" in self.db and "torch" in self.db:
            worst, differ, total = 0.0, 0, 0
            for side, x in self.batches["color"].items():
                d = (x.float() - self.mixed[side].float()).abs()
                worst, differ, total = max(worst, float(d.max())), differ + int((d != 0).sum()), total + d.numel()
            # (f16 values up to (255 - 0.406 * 255) / (0.225 * 255) = 2.64: one unit in the last place there is 2^-9)
            assert worst <= 2.0 ** -9 * 1.001, f"torch's batches differ from the colour call's by {worst}, more than one last place of f16"
            notes.append(f"torch differs from color in {100.0 * differ / total:.2f} % of the elements, by at most {worst:.6f} (one last place of f16 at 2 .. 4 is {2.0 ** -9:.6f})")
        return notes


def overlap(a, b):
    return "do not overlap" if max(a) < min(b) or max(b) < min(a) else "OVERLAP"


def time_mode(rounds, steps, n):
    enc = fpng_amd.Encoder(device=0)
    dev = files_on_device(enc, W, H, n)
    for key in WORKLOADS:
        s = Sides(enc, dev, key)
        print(f"workload {key}: {n} x 1080p RGB, {s.v} views per file -> f16, a colour matrix per view", flush=True)
        for note in s.check():
            print(f"    {note}", flush=True)
        for name in s.db:
            window(lambda: s.run(name), 3)
        t = {name: [] for name in s.db}
        for _ in range(rounds):
            for name in s.db:
                t[name].append(window(lambda: s.run(name), steps))
        for name in t:
            print(f"    {name:10s} {spread(t[name])} per call, {rounds} rounds x {steps} calls", flush=True)
        m = {name: statistics.median(t[name]) for name in t}
        for name in ("color", "color_hwc"):
            print(f"    {name} / torch = {m[name] / m['torch']:.3f} ({m['torch'] - m[name]:+.4f} ms saved; ranges {overlap(t[name], t['torch'])});  "
                  f"{name} / plain = {m[name] / m['plain']:.3f} ({m[name] - m['plain']:+.4f} ms over the floor; ranges {overlap(t[name], t['plain'])})", flush=True)
        enc.set_profiling(True)
        ph = {name: [] for name in s.db}
        for _ in range(5):
            for name in s.db:
                s.run(name)
                torch.cuda.synchronize()
                ph[name].append(enc.last_decode_phase_ms())
        enc.set_profiling(False)
        for name in ph:
            med = {k: statistics.median(p[k] for p in ph[name]) for k in ph[name][0]}
            print(f"    {name:10s} phases of the decode call (ms): " + ", ".join(f"{k} {v:.3f}" for k, v in med.items()) +
                  f"; behind the synchronisation (pixel pass + resize) {100.0 * med['unfilter'] / sum(med.values()):.0f} % of them", flush=True)
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
