#!/usr/bin/env python
"""What the per-view tone stage of the views call (fpng_amd_decode_batch_device_planar_views_tone: autocontrast, equalize, contrast
about the view's own mean) costs against what a user does without it -- the views call to uint8 batches, then torch for the
per-sample histograms, tables, look-up, normalisation and cast -- and against the same call with tone=None, the floor; one box, one
process (a sibling of tools/views_post_timing.py, whose workloads, files, window, rounds and steps it uses).

    python tools/views_tone_timing.py time   [rounds] [steps] [files]
    python tools/views_tone_timing.py kernel <a|b> <tone|torch|plain|solid|solid_plain> [calls] [files]

256 device-resident 1080p RGB files, f16 with ImageNet's mean / std, every second view mirrored; workloads a and b of views_timing.py;
one tone operation drawn per view: autocontrast, equalize and contrast (factor 0.1 .. 1.9) in turn, so all three are represented.
One batch per view size: (files x views of that size, 3, side, side).
  tone         the tone call: histograms, tables, look-up, normalisation, cast in the one call
  torch        the views call to uint8 batches, then per batch a restatement of the rule in plain torch: bincount for
               the per-sample histograms of R, G, B and L, the three rules' tables for every sample and where() for the drawn one,
               gather for the look-up, the normalisation's multiply and add, the cast to f16.  It follows the rule exactly, so its
               batches are compared with the tone call's: the same bytes, hence at most a last place of f16 apart
  plain        the same call with tone=None: the floor
  solid        the tone call on SOLID views (a colour matrix that zeroes the input): every sample of a wave goes to one LDS address
  solid_plain  the colour call with that matrix and no tone: the floor of solid
time    The sides take turns round by round; a window is `steps` back-to-back calls between two device events, after a warm-up of
        all; the median window per call with its min-max over the rounds, then the phases of the decode call
        (last_decode_phase_ms under set_profiling: "unfilter" brackets the pixel pass, the resize, the tone kernels and the post stage).
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
from views_color_timing import overlap  # noqa: E402
from views_timing import WORKLOADS, random_resized_crop, spread  # noqa: E402

SIDES = ("tone", "torch", "plain", "solid", "solid_plain")
SOLID = np.array([[0, 0, 0, 77], [0, 0, 0, 130], [0, 0, 0, 255]], dtype=np.float32)


class Sides:
    """the descriptors of one workload: the same crops, views, tone records and constants; a batch per view size and side"""

    def __init__(self, enc, dev, key, which=SIDES):
        n, spec = len(dev), WORKLOADS[key]
        rng = np.random.default_rng(2024)
        self.enc, self.key, self.n, self.v = enc, key, n, len(spec)
        crops = [[random_resized_crop(rng, scale) for _, scale in spec] for _ in range(n)]
        fulls = [[(side, side) for side, _ in spec] for _ in range(n)]
        mirrors = [[bool(k & 1) for k in range(len(spec))] for _ in range(n)]
        # (op, factor) of view k of file i: the three operations in turn
        draws = [[((i * len(spec) + k) % 3 + 1, float(np.float32(rng.uniform(0.1, 1.9)))) for k in range(len(spec))] for i in range(n)]
        tones = [[fpng_amd.view_tone(autocontrast=op == 1, equalize=op == 2, contrast=f if op == 3 else None) for op, f in ds] for ds in draws]
        per_size = {side: sum(s == side for s, _ in spec) for side, _ in spec}
        slot, seen = [], {}
        for side, _ in spec:  # view k of a file is image number slot[k] of its size among the file's
            slot.append(seen.get(side, 0))
            seen[side] = slot[-1] + 1
        self.batches, self.db, self.done = {}, {}, {}
        for name in which:
            u8 = name == "torch"
            x = {side: torch.empty((n * cnt, 3, side, side), dtype=torch.uint8 if u8 else torch.float16, device="cuda") for side, cnt in per_size.items()}
            outs = [[x[side][i * per_size[side] + slot[k]] for k, (side, _) in enumerate(spec)] for i in range(n)]
            kw = {} if u8 else {"mean": MEAN, "std": STD}
            if name in ("tone", "solid"):
                kw["tone"] = tones
            if name.startswith("solid"):
                kw["color"] = SOLID
            self.db[name] = enc.make_decode_batch_views(dev, crops, outs, fulls, mirror=mirrors, **kw)
            self.batches[name] = x
        # the torch side's constants: per batch the samples' operations and factors
        self.op, self.factor = {}, {}
        for side, cnt in per_size.items():
            op, factor = np.zeros(n * cnt, dtype=np.int64), np.zeros(n * cnt, dtype=np.float32)
            for i in range(n):
                for k, (s, _) in enumerate(spec):
                    if s == side:
                        op[i * cnt + slot[k]], factor[i * cnt + slot[k]] = draws[i][k]
            self.op[side], self.factor[side] = torch.from_numpy(op).cuda().view(-1, 1, 1), torch.from_numpy(factor).cuda().view(-1, 1, 1)
        scale, bias = fpng_amd.normalize_constants(MEAN, STD)
        self.scale = torch.tensor([float(v) for v in scale[:3]], dtype=torch.float32, device="cuda").view(1, 3, 1, 1)
        self.bias = torch.tensor([float(v) for v in bias[:3]], dtype=torch.float32, device="cuda").view(1, 3, 1, 1)
        self.v256 = torch.arange(256, device="cuda").view(1, 1, 256)

    def tables(self, x, op, factor):
        """(N, 3, 256) int64 tables of the batch x (N, 3, S, S) uint8 by the rule of include/fpng_amd.h"""
        n, count = x.shape[0], x.shape[2] * x.shape[3]
        xi = x.view(n, 3, -1).long()
        h = torch.bincount((xi + 256 * torch.arange(n * 3, device="cuda").view(n, 3, 1)).flatten(), minlength=n * 3 * 256).view(n, 3, 256)
        lum = (19595 * xi[:, 0] + 38470 * xi[:, 1] + 7471 * xi[:, 2] + 0x8000) >> 16
        hl = torch.bincount((lum + 256 * torch.arange(n, device="cuda").view(n, 1)).flatten(), minlength=n * 256).view(n, 1, 256)
        v = self.v256
        nz = (h > 0).long()
        lo, hi = nz.argmax(-1, keepdim=True), 255 - nz.flip(-1).argmax(-1, keepdim=True)
        span = (hi - lo).clamp(min=1).double()
        scale = torch.full_like(span, 255.0) / span  # (a division: 255.0 / tensor is a reciprocal and a product, an ulp off at times)
        auto = torch.where(hi > lo, (v.double() * scale + (-lo.double() * scale)).trunc().clamp(0, 255).long(), v.expand_as(h))
        step = (h.sum(-1, keepdim=True) - h.gather(-1, hi)) // 255
        equal = torch.where(step > 0, ((step // 2 + h.cumsum(-1) - h) // step.clamp(min=1)).clamp(max=255), v.expand_as(h))
        mean = (2 * (v * hl).sum(-1, keepdim=True) + count) // (2 * count)
        contrast = (mean.float() + factor * (v - mean).float()).clamp(0.0, 255.0).trunc().long().expand_as(h)
        return torch.where(op == 1, auto, torch.where(op == 2, equal, contrast))

    def run(self, name):
        self.enc.decode_device_views(self.db[name], results=False)
        if name != "torch":
            return
        for side, x in self.batches[name].items():  # (what the tone call replaces: on the same stream, behind the decode)
            lut = self.tables(x, self.op[side], self.factor[side])
            y = lut.gather(-1, x.view(x.shape[0], 3, -1).long()).view(x.shape).float()  # look-up, convert
            y.mul_(self.scale).add_(self.bias)                                          # normalise
            self.done[side] = y.to(torch.float16)                                       # cast

    def check(self):
        for name in self.db:
            self.run(name)
        torch.cuda.synchronize()
        assert all(s == 0 for d in self.db.values() for s in d.statuses())
        notes = []
        if "tone" in self.db and "torch" in self.db:
            worst, differ, total = 0.0, 0, 0
            for side, x in self.batches["tone"].items():
                d = (x.float() - self.done[side].float()).abs()
                worst, differ, total = max(worst, float(d.max())), differ + int((d != 0).sum()), total + d.numel()
            # (torch follows the rule, so the bytes are the same; it normalises with a multiply and an add, rounded twice, where the
            #  call has one fused multiply-add, and both then round to f16: 2^-9 apart at 2 .. 4.  One byte would be 1 / (0.225 * 255))
            step = 1.0 / (min(STD) * 255.0)
            notes.append(f"torch differs from tone in {100.0 * differ / total:.3f} % of the elements, by at most {worst:.5f} (a last place of f16 at 2 .. 4 is {2.0 ** -9:.5f}; one byte is {step:.5f})")
        if "tone" in self.db and "plain" in self.db:
            same = all(torch.equal(x.view(torch.int16), self.batches["plain"][side].view(torch.int16)) for side, x in self.batches["tone"].items())
            notes.append("tone and plain differ (the tone stage does something)" if not same else "tone and plain are the same: NO view has an op")
        return notes


def time_mode(rounds, steps, n):
    enc = fpng_amd.Encoder(device=0)
    dev = files_on_device(enc, W, H, n)
    for key in WORKLOADS:
        s = Sides(enc, dev, key)
        print(f"workload {key}: {n} x 1080p RGB, {s.v} views per file -> f16, one tone operation per view (autocontrast, equalize, contrast in turn)", flush=True)
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
        print(f"    tone / torch = {m['tone'] / m['torch']:.3f} ({m['torch'] - m['tone']:+.4f} ms saved; ranges {overlap(t['tone'], t['torch'])});  "
              f"tone - plain = {m['tone'] - m['plain']:+.4f} ms, the price of the tone stage (tone / plain = {m['tone'] / m['plain']:.3f}; ranges {overlap(t['tone'], t['plain'])})", flush=True)
        print(f"    solid - solid_plain = {m['solid'] - m['solid_plain']:+.4f} ms against tone - plain = {m['tone'] - m['plain']:+.4f} ms: what one LDS address per wave costs "
              f"(ranges of solid and tone {overlap(t['solid'], t['tone'])})", flush=True)
        enc.set_profiling(True)
        ph = {name: [] for name in s.db}
        for _ in range(5):
            for name in s.db:
                s.run(name)
                torch.cuda.synchronize()
                ph[name].append(enc.last_decode_phase_ms())
        enc.set_profiling(False)
        med = {name: {k: statistics.median(p[k] for p in ph[name]) for k in ph[name][0]} for name in ph}
        for name in ph:
            print(f"    {name:11s} phases of the decode call (ms): " + ", ".join(f"{k} {v:.3f}" for k, v in med[name].items()), flush=True)
        extra = med["tone"]["unfilter"] - med["plain"]["unfilter"]
        print(f"    the tone stage (the windows into the scratch, the two tone kernels and dec_view_post_kernel): {extra:+.3f} ms of the phase behind the synchronisation, "
              f"{100.0 * extra / sum(med['tone'].values()):.0f} % of the tone call's phases", flush=True)
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
