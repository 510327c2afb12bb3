#!/usr/bin/env python
"""What the per-view post stage of the views call (fpng_amd_decode_batch_device_planar_views_post: Gaussian blur, solarize) costs
against what a user does without it -- the colour call to uint8 batches, then torch for the per-sample blur, the solarize, the
normalisation and the cast -- and against the colour call to f16 with no post stage at all, the floor; one box, one process (a
sibling of tools/views_color_timing.py, whose workloads, files, matrices, window, rounds and steps it uses).

    python tools/views_post_timing.py time   [rounds] [steps] [files]
    python tools/views_post_timing.py kernel <a|b> <post|torch|color> [calls] [files]

256 device-resident 1080p RGB files, f16 with ImageNet's mean / std, every second view mirrored; workloads a and b of views_timing.py;
every view its own colour matrix; the BYOL-style draw of the post step: GaussianBlur(23, sigma 0.1 .. 2.0) on the first 224 x 224
view always, on the second with probability 0.1 and on a 96 x 96 view with probability 0.5, solarize(128) on one view in five.
One batch per view size: (files x views of that size, 3, side, side).
  post    the post call: colour matrix, blur, solarize, normalisation, cast in the one call
  torch   the colour call to uint8 batches, then per batch: the blurred samples gathered, converted, padded (reflect), two grouped
          conv2d with a kernel per sample, rounded, clamped, scattered back; where() for the solarized samples; the
          normalisation's multiply and add; the cast to f16
  color   the colour call to f16 with no post step: the floor
time    The sides take turns round by round; a window is `steps` back-to-back calls between two device events, after a warm-up of
        all; the median window per call with its min-max over the rounds, then the phases of the decode call
        (last_decode_phase_ms under set_profiling: "unfilter" brackets the pixel pass, the resize and the post stage).  Before
        timing, torch is compared with post: the same bytes give or take 1 (torch sums in float and rounds once).
kernel  `calls` calls of one side of one workload and nothing else: run it under `rocprofv3 --kernel-trace --stats`."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fpng_amd  # noqa: E402  (before the first torch.cuda call: the library sets the hardware queue count)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from resize_decode_timing import H, MEAN, STD, W, window  # noqa: E402
from resize_view_timing import files_on_device  # noqa: E402
from views_color_timing import jitter, overlap  # noqa: E402
from views_timing import WORKLOADS, random_resized_crop, spread  # noqa: E402

SIDES = ("post", "torch", "color")
RADIUS = 11  # GaussianBlur(kernel_size=23)


def draw(rng, k, side):
    """the post step of view k of a file: (sigma or None, solarize?)"""
    p_blur = 0.5 if side != 224 else (1.0, 0.1)[k & 1]
    sigma = float(rng.uniform(0.1, 2.0)) if rng.random() < p_blur else None
    return sigma, bool(rng.random() < 0.2)


class Sides:
    """the descriptors of one workload: the same crops, views, matrices, post steps and constants; a batch per view size and side"""

    def __init__(self, enc, dev, key, which=SIDES):
        n, spec = len(dev), WORKLOADS[key]
        rng = np.random.default_rng(2024)
        self.enc, self.key, self.n, self.v = enc, key, n, len(spec)
        crops = [[random_resized_crop(rng, scale) for _, scale in spec] for _ in range(n)]
        fulls = [[(side, side) for side, _ in spec] for _ in range(n)]
        mirrors = [[bool(k & 1) for k in range(len(spec))] for _ in range(n)]
        colors = [[jitter(rng) for _ in spec] for _ in range(n)]
        draws = [[draw(rng, k, side) for k, (side, _) in enumerate(spec)] for _ in range(n)]
        posts = [[fpng_amd.view_post(blur=None if sigma is None else (2 * RADIUS + 1, sigma), solarize=128 if sol else None) for sigma, sol in ds] for ds in draws]
        per_size = {side: sum(s == side for s, _ in spec) for side, _ in spec}
        slot, seen = [], {}
        for side, _ in spec:  # view k of a file is image number slot[k] of its size among the file's
            slot.append(seen.get(side, 0))
            seen[side] = slot[-1] + 1
        self.blurred = sum(sigma is not None for ds in draws for sigma, _ in ds) / (n * len(spec))
        self.solarized = sum(sol for ds in draws for _, sol in ds) / (n * len(spec))
        self.batches, self.db, self.done = {}, {}, {}
        for name in which:
            u8 = name == "torch"
            x = {side: torch.empty((n * cnt, 3, side, side), dtype=torch.uint8 if u8 else torch.float16, device="cuda") for side, cnt in per_size.items()}
            outs = [[x[side][i * per_size[side] + slot[k]] for k, (side, _) in enumerate(spec)] for i in range(n)]
            kw = {"color": colors} if u8 else {"color": colors, "mean": MEAN, "std": STD}
            if name == "post":
                kw["post"] = posts
            self.db[name] = enc.make_decode_batch_views(dev, crops, outs, fulls, mirror=mirrors, **kw)
            self.batches[name] = x
        # the torch side's constants: per batch the blurred samples' numbers and kernels, the solarized samples' mask
        self.blur_at, self.taps, self.sol = {}, {}, {}
        for side, cnt in per_size.items():
            at, taps, sol = [], [], np.zeros((n * cnt, 1, 1, 1), dtype=bool)
            for i in range(n):
                for k, (s, _) in enumerate(spec):
                    if s != side:
                        continue
                    sigma, solarize = draws[i][k]
                    sol[i * cnt + slot[k]] = solarize
                    if sigma is not None:
                        d = np.arange(-RADIUS, RADIUS + 1, dtype=np.float64)
                        p = np.exp(-0.5 * (d / sigma) ** 2)
                        at.append(i * cnt + slot[k]), taps.append(np.repeat((p / p.sum())[None, :], 3, axis=0))
            self.blur_at[side] = torch.tensor(at, dtype=torch.int64, device="cuda")
            self.taps[side] = torch.from_numpy(np.concatenate(taps).astype(np.float32)).cuda() if taps else None  # (blurred samples x 3, 23)
            self.sol[side] = torch.from_numpy(sol).cuda()
        scale, bias = fpng_amd.normalize_constants(MEAN, STD)
        self.scale = torch.tensor([float(v) for v in scale[:3]], dtype=torch.float32, device="cuda").view(1, 3, 1, 1)
        self.bias = torch.tensor([float(v) for v in bias[:3]], dtype=torch.float32, device="cuda").view(1, 3, 1, 1)

    def run(self, name):
        self.enc.decode_device_views(self.db[name], results=False)
        if name != "torch":
            return
        for side, x in self.batches[name].items():  # (what the post call replaces: on the same stream, behind the decode)
            at, taps = self.blur_at[side], self.taps[side]
            if taps is not None:
                g = x.index_select(0, at).float().view(1, -1, side, side)                                    # gather, convert
                g = F.pad(g, (RADIUS, RADIUS, RADIUS, RADIUS), mode="reflect")                               # pad
                g = F.conv2d(g, taps.view(-1, 1, 1, 2 * RADIUS + 1), groups=taps.shape[0])                   # a kernel per sample: rows
                g = F.conv2d(g, taps.view(-1, 1, 2 * RADIUS + 1, 1), groups=taps.shape[0])                   # ... columns
                x.index_copy_(0, at, g.round_().clamp_(0.0, 255.0).to(torch.uint8).view(-1, 3, side, side))  # round, clamp, scatter
            y = torch.where(self.sol[side] & (x >= 128), 255 - x, x).float()                                 # solarize, convert
            y.mul_(self.scale).add_(self.bias)                                                               # normalise
            self.done[side] = y.to(torch.float16)                                                            # cast

    def check(self):
        for name in self.db:
            self.run(name)
        torch.cuda.synchronize()
        assert all(s == 0 for d in self.db.values() for s in d.statuses())
        notes = [f"{100 * self.blurred:.0f} % of the views blurred, {100 * self.solarized:.0f} % solarized"]
        if "post" in self.db and "torch" in self.db:
            worst, differ, total = 0.0, 0, 0
            for side, x in self.batches["post"].items():
                d = (x.float() - self.done[side].float()).abs()
                worst, differ, total = max(worst, float(d.max())), differ + int((d != 0).sum()), total + d.numel()
            # (one byte is 1 / (0.225 * 255) = 0.0174 after the normalisation, and both sides round to f16 there: 2^-9 at 2 .. 4)
            step = 1.0 / (min(STD) * 255.0)
            assert worst <= step + 2.0 ** -8, f"torch's batches differ from the post call's by {worst}, more than one byte ({step:.4f}) and the roundings to f16"
            notes.append(f"torch differs from post in {100.0 * differ / total:.2f} % of the elements, by at most {worst:.5f} (one byte is {step:.5f})")
        if "post" in self.db and "color" in self.db:
            same = all(torch.equal(x.view(torch.int16), self.batches["color"][side].view(torch.int16)) for side, x in self.batches["post"].items())
            notes.append("post and color differ (the post step does something)" if not same else "post and color are the same: NO view has a post step")
        return notes


def time_mode(rounds, steps, n):
    enc = fpng_amd.Encoder(device=0)
    dev = files_on_device(enc, W, H, n)
    for key in WORKLOADS:
        s = Sides(enc, dev, key)
        print(f"workload {key}: {n} x 1080p RGB, {s.v} views per file -> f16, a colour matrix and a post record per view", flush=True)
        for note in s.check():
            print(f"    {note}", flush=True)
        for name in s.db:
            window(lambda: s.run(name), 3)
        t = {name: [] for name in s.db}
        for _ in range(rounds):
            for name in s.db:
                t[name].append(window(lambda: s.run(name), steps))
        for name in t:
            print(f"    {name:6s} {spread(t[name])} per call, {rounds} rounds x {steps} calls", flush=True)
        m = {name: statistics.median(t[name]) for name in t}
        print(f"    post / torch = {m['post'] / m['torch']:.3f} ({m['torch'] - m['post']:+.4f} ms saved; ranges {overlap(t['post'], t['torch'])});  "
              f"post - color = {m['post'] - m['color']:+.4f} ms, the price of the post stage (post / color = {m['post'] / m['color']:.3f}; ranges {overlap(t['post'], t['color'])})", flush=True)
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
            print(f"    {name:6s} phases of the decode call (ms): " + ", ".join(f"{k} {v:.3f}" for k, v in med[name].items()) +
                  f"; behind the synchronisation (pixel pass + resize + post) {100.0 * med[name]['unfilter'] / sum(med[name].values()):.0f} % of them", flush=True)
        extra = med["post"]["unfilter"] - med["color"]["unfilter"]
        print(f"    the post stage (the windows into the scratch and dec_view_post_kernel): {extra:+.3f} ms of that phase, {100.0 * extra / sum(med['post'].values()):.0f} % of the post call's phases",
              flush=True)
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
