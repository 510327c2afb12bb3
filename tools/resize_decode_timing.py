#!/usr/bin/env python
"""What decoding a crop of each file RESIZED to a fixed size costs against what a loader did before it -- decode_device_crop to uint8
tensors of n different sizes, then per file F.interpolate(bilinear, antialias), flip, normalise and a copy into the batch -- on the
same box in one process.

    python tools/resize_decode_timing.py [rounds] [steps] [files]

256 device-resident 1080p RGB files (four distinct `grad` images, repeated), seeded RandomResizedCrop boxes (area 0.08 ... 1 of the
image, aspect ratio 3/4 ... 4/3, log-uniform), every second file mirrored, into one (n, 3, 224, 224) f16 batch with ImageNet's
mean / std.  Descriptors and the baseline's odd-sized tensors are built once.  The variants take turns round by round; a window is
`steps` back-to-back calls between two device events on the encoder's stream, after a warm-up of every variant; the median window is
reported per call with its min-max over the rounds.  Variants:
  a   decode_device_crop to uint8, then per file interpolate / flip / normalise / copy into the batch: the path that was there before
  b   decode_device_resize into the views of the batch
  c   decode_device_crop to uint8 alone (b's first stage into caller memory; a without its torch passes)
The resize kernel's own time: the encoder's profiling events (set_profiling) bracket the kernels behind the synchronisation -- the
pixel pass, and in b the resize behind it; b's bracket minus c's is the resize stage.
b is checked first against a: the two resamplers differ (a: float, torch's antialiased bilinear; b: Pillow's 8-bit rule), so the
check is that the mean absolute difference is below one byte step (1 / 255 / std) -- a gross error (wrong crop, missing flip) fails it."""
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fpng_amd  # noqa: E402  (before the first torch.cuda call: the library sets the hardware queue count)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
W, H, SIDE = 1920, 1080, 224


def window(fn, m):
    """ms per call of m back-to-back calls, between two device events on the current stream"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(m):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / m


def random_resized_crop(rng):
    """torchvision's RandomResizedCrop.get_params: ten tries, then the central crop"""
    for _ in range(10):
        area = W * H * rng.uniform(0.08, 1.0)
        ratio = math.exp(rng.uniform(math.log(3 / 4), math.log(4 / 3)))
        cw, ch = int(round(math.sqrt(area * ratio))), int(round(math.sqrt(area / ratio)))
        if 0 < cw <= W and 0 < ch <= H:
            return int(rng.integers(0, W - cw + 1)), int(rng.integers(0, H - ch + 1)), cw, ch
    return (W - H) // 2, 0, H, H


def main():
    nums = [int(a) for a in sys.argv[1:] if a.isdigit()]
    rounds, steps, n = (nums + [7, 10, 256][len(nums):])[:3]
    assert torch.cuda.is_available(), "this tool measures on a GPU"
    print(f"{torch.cuda.get_device_name(0)}, torch {torch.__version__}, hip {torch.version.hip}", flush=True)
    enc = fpng_amd.Encoder(device=0)
    pngs = []
    for i in range(4):
        (p,), _ = enc.encode_tensors([torch.from_numpy(fpng_amd.synth_image("grad", W, H, 3, seed=12345 + i)).cuda()], 0)
        pngs.append(p)
    dev = [torch.frombuffer(bytearray(pngs[i % 4]), dtype=torch.uint8).cuda() for i in range(n)]
    rng = np.random.default_rng(2024)
    crops = [random_resized_crop(rng) for _ in range(n)]
    mirrors = [bool(i & 1) for i in range(n)]
    odd = [torch.empty((3, ch, cw), dtype=torch.uint8, device="cuda") for _, _, cw, ch in crops]
    batch_a = torch.empty((n, 3, SIDE, SIDE), dtype=torch.float16, device="cuda")
    batch_b = torch.empty((n, 3, SIDE, SIDE), dtype=torch.float16, device="cuda")
    crop = enc.make_decode_batch_crop(dev, crops, odd)
    resize = enc.make_decode_batch_resize(dev, crops, list(batch_b), mirror=mirrors, mean=MEAN, std=STD)
    mean = torch.tensor(MEAN, device="cuda")[:, None, None]
    std = torch.tensor(STD, device="cuda")[:, None, None]

    def dec_a():
        enc.decode_device_crop(crop, results=False)
        for i, t in enumerate(odd):
            x = F.interpolate(t[None].float(), size=(SIDE, SIDE), mode="bilinear", antialias=True)[0]
            if mirrors[i]:
                x = x.flip(2)
            batch_a[i] = (x / 255.0 - mean) / std

    def dec_b():
        enc.decode_device_resize(resize, results=False)

    def dec_c():
        enc.decode_device_crop(crop, results=False)
    v = {"a": dec_a, "b": dec_b, "c": dec_c}
    for fn in v.values():
        fn()
    torch.cuda.synchronize()
    assert all(s == 0 for d in (crop, resize) for s in d.statuses())
    diff = (batch_a.float() - batch_b.float()).abs()
    step = 1.0 / 255.0 / min(STD)
    print(f"b against a: mean |difference| {float(diff.mean()):.5f}, max {float(diff.max()):.5f} (one byte step: {step:.5f})", flush=True)
    assert float(diff.mean()) < step, "the new call's batch is not the baseline's"
    for fn in v.values():
        window(fn, 3)
    t = {key: [] for key in v}
    for _ in range(rounds):
        for key, fn in v.items():
            t[key].append(window(fn, steps))
    med = {key: statistics.median(t[key]) for key in t}
    print(f"{n} x 1080p RGB, RandomResizedCrop boxes -> {SIDE}x{SIDE} f16, {rounds} rounds x {steps} calls: median ms per call (min-max)", flush=True)
    for key in t:
        print(f"    {key}  {med[key]:8.4f} ms ({min(t[key]):.4f}-{max(t[key]):.4f})", flush=True)
    print(f"    b / a = {med['b'] / med['a']:.3f}   b < a, ranges apart: {'YES' if max(t['b']) < min(t['a']) else 'NO'}", flush=True)
    # the kernels behind the synchronisation, by the encoder's own events: b (pixel pass + resize) and c (pixel pass)
    enc.set_profiling(True)
    ph = {"b": [], "c": []}
    for _ in range(rounds):
        for key in ph:
            v[key]()
            torch.cuda.synchronize()
            ph[key].append(enc.last_decode_phase_ms()["unfilter"])
    enc.set_profiling(False)
    pb, pc = statistics.median(ph["b"]), statistics.median(ph["c"])
    print(f"    kernels behind the synchronisation: b {pb:.4f} ms ({min(ph['b']):.4f}-{max(ph['b']):.4f}), c {pc:.4f} ms ({min(ph['c']):.4f}-{max(ph['c']):.4f})", flush=True)
    print(f"    the resize stage (b - c): {pb - pc:.4f} ms for {n} files x 3 planes", flush=True)
    enc.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
