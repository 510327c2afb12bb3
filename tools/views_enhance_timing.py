#!/usr/bin/env python
"""What the per-view enhance stage of the views call (fpng_amd_decode_batch_device_planar_views_enhance: brightness, color,
sharpness) costs on top of the tone call: the batch of tools/views_tone_timing.py -- its files, crops, views, tone records and
constants -- once through the _views_tone call, the code path of the call without enhance=, and once with an enhance record on
every view; one box, one process (a sibling of tools/views_tone_timing.py, whose workloads, window, rounds and steps it uses).

    python tools/views_enhance_timing.py time [rounds] [steps] [files]

256 device-resident 1080p RGB files, f16 with ImageNet's mean / std, every second view mirrored; workloads a and b of views_timing.py;
one tone operation per view as the tone tool draws them.
  tone        the tone call (no enhance=): the floor, and the parent's code path
  sharpness   the same with view_enhance(sharpness=factor) on every view, factor 0.1 .. 1.9: the dearest operation (a halo, a 3 x 3
              filter in LDS)
  color       the same with view_enhance(color=factor) on every view
  brightness  the same with view_enhance(brightness=factor) on every view
The sides take turns round by round; a window is `steps` back-to-back calls between two device events, after a warm-up of all; the
median window per call with its min-max over the rounds, and each side's ratio to the tone call."""
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
from views_color_timing import overlap  # noqa: E402
from views_timing import WORKLOADS, random_resized_crop, spread  # noqa: E402

SIDES = ("tone", "sharpness", "color", "brightness")


class Sides:
    """the descriptors of one workload: the same crops, views, tone records and constants; a batch per view size and side"""

    def __init__(self, enc, dev, key):
        n, spec = len(dev), WORKLOADS[key]
        rng = np.random.default_rng(2024)
        self.enc, self.n, self.v = enc, n, len(spec)
        crops = [[random_resized_crop(rng, scale) for _, scale in spec] for _ in range(n)]
        fulls = [[(side, side) for side, _ in spec] for _ in range(n)]
        mirrors = [[bool(k & 1) for k in range(len(spec))] for _ in range(n)]
        # (views_tone_timing.py's draws: the three tone operations in turn)
        draws = [[((i * len(spec) + k) % 3 + 1, float(np.float32(rng.uniform(0.1, 1.9)))) for k in range(len(spec))] for i in range(n)]
        tones = [[fpng_amd.view_tone(autocontrast=op == 1, equalize=op == 2, contrast=f if op == 3 else None) for op, f in ds] for ds in draws]
        per_size = {side: sum(s == side for s, _ in spec) for side, _ in spec}
        slot, seen = [], {}
        for side, _ in spec:  # view k of a file is image number slot[k] of its size among the file's
            slot.append(seen.get(side, 0))
            seen[side] = slot[-1] + 1
        self.batches, self.db = {}, {}
        for name in SIDES:
            x = {side: torch.empty((n * cnt, 3, side, side), dtype=torch.float16, device="cuda") for side, cnt in per_size.items()}
            outs = [[x[side][i * per_size[side] + slot[k]] for k, (side, _) in enumerate(spec)] for i in range(n)]
            kw = {"mean": MEAN, "std": STD, "tone": tones}
            if name != "tone":
                kw["enhance"] = [[fpng_amd.view_enhance(**{name: f}) for _, f in ds] for ds in draws]
            self.db[name] = enc.make_decode_batch_views(dev, crops, outs, fulls, mirror=mirrors, **kw)
            self.batches[name] = x

    def run(self, name):
        self.enc.decode_device_views(self.db[name], results=False)

    def check(self):
        for name in self.db:
            self.run(name)
        torch.cuda.synchronize()
        assert all(s == 0 for d in self.db.values() for s in d.statuses())
        notes = []
        for name in SIDES[1:]:
            same = all(torch.equal(x.view(torch.int16), self.batches["tone"][side].view(torch.int16)) for side, x in self.batches[name].items())
            notes.append(f"{name} and tone differ (the stage does something)" if not same else f"{name} and tone are the same: NO view has an op")
        return notes


def time_mode(rounds, steps, n):
    enc = fpng_amd.Encoder(device=0)
    dev = files_on_device(enc, W, H, n)
    for key in WORKLOADS:
        s = Sides(enc, dev, key)
        print(f"workload {key}: {n} x 1080p RGB, {s.v} views per file -> f16, one tone operation per view, one enhance operation per view but for `tone`", flush=True)
        for note in s.check():
            print(f"    {note}", flush=True)
        for name in s.db:
            window(lambda: s.run(name), 3)
        t = {name: [] for name in s.db}
        for _ in range(rounds):
            for name in s.db:
                t[name].append(window(lambda: s.run(name), steps))
        for name in t:
            print(f"    {name:11s} {spread(t[name])} per call, {rounds} rounds x {steps} calls", flush=True)
        m = {name: statistics.median(t[name]) for name in t}
        for name in SIDES[1:]:
            print(f"    {name} / tone = {m[name] / m['tone']:.3f} ({m[name] - m['tone']:+.4f} ms, the price of the stage; ranges {overlap(t[name], t['tone'])})", flush=True)
        del s
    enc.close()


def main():
    nums = [int(a) for a in sys.argv[2:] if a.isdigit()]
    if len(sys.argv) < 2 or sys.argv[1] != "time":
        print(__doc__)
        return 2
    rounds, steps, n = (nums + [9, 10, 256][len(nums):])[:3]
    assert torch.cuda.is_available(), "this tool measures on a GPU"
    print(f"{torch.cuda.get_device_name(0)}, torch {torch.__version__}, hip {torch.version.hip}", flush=True)
    time_mode(rounds, steps, n)
    return 0


if __name__ == "__main__":
    sys.exit(main())
