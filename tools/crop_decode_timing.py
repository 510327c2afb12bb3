#!/usr/bin/env python
"""What decoding a CROP of each file costs against what a loader did before it -- decode_device_float into full-size tensors, then
torch.stack of the slices -- on the same box in one process.

    python tools/crop_decode_timing.py [rounds] [steps] [workload ...]

Device-resident files (four distinct `grad` images per workload, repeated), seeded random crop positions, descriptors built once.
The variants take turns round by round; a window is `steps` back-to-back calls between two device events on the encoder's stream,
after a warm-up of every variant; the median window is reported per call with its min-max over the rounds.  Variants:
  a   decode_device_float into full-size (c, h, w) tensors, then torch.stack([t[:, y:y+h, x:x+w] ...]).contiguous(): the path that
      was there before
  b   decode_device_crop into the views of one (n, c, crop h, crop w) tensor
  f   decode_device_float alone (the full decode: a without its copy)
  c   decode_device_crop with the WHOLE image as the crop: what the clipping costs when nothing is dropped (against f)
b's elements are checked first against a's, bit for bit.  Workloads: 256 x 512^2 RGB -> 224^2 f16, 64 x 1080p RGB -> 224^2 f16,
8 x 8K RGBA -> 1024^2 f32."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fpng_amd  # noqa: E402  (before the first torch.cuda call: the library sets the hardware queue count)
import numpy as np  # noqa: E402
import torch  # noqa: E402

MEAN, STD = (0.485, 0.456, 0.406, 0.5), (0.229, 0.224, 0.225, 0.25)
WORKLOADS = {"512": ("256 x 512x512 RGB -> 224x224 f16", 512, 512, 3, 256, 224, torch.float16),
             "1080p": ("64 x 1080p RGB -> 224x224 f16", 1920, 1080, 3, 64, 224, torch.float16),
             "8k": ("8 x 8K RGBA -> 1024x1024 f32", 7680, 4320, 4, 8, 1024, torch.float32)}


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


def workload(enc, name, w, h, c, n, side, dtype, rounds, steps):
    pngs = []
    for i in range(4):
        (p,), _ = enc.encode_tensors([torch.from_numpy(fpng_amd.synth_image("grad", w, h, c, seed=12345 + i)).cuda()], 0)
        pngs.append(p)
    dev = [torch.frombuffer(bytearray(pngs[i % 4]), dtype=torch.uint8).cuda() for i in range(n)]
    rng = np.random.default_rng(2024)
    crops = [(int(rng.integers(0, w - side + 1)), int(rng.integers(0, h - side + 1)), side, side) for _ in range(n)]
    whole = torch.empty((n, c, h, w), dtype=dtype, device="cuda")
    batch = torch.empty((n, c, side, side), dtype=dtype, device="cuda")
    whole2 = torch.empty((n, c, h, w), dtype=dtype, device="cuda")
    full = enc.make_decode_batch_float(dev, list(whole), mean=MEAN[:c], std=STD[:c])
    crop = enc.make_decode_batch_crop(dev, crops, list(batch), mean=MEAN[:c], std=STD[:c])
    crop_all = enc.make_decode_batch_crop(dev, [(0, 0, w, h)] * n, list(whole2), mean=MEAN[:c], std=STD[:c])
    keep = {}

    def dec_a():
        enc.decode_device_float(full, results=False)
        keep["a"] = torch.stack([whole[i, :, y:y + ch, x:x + cw] for i, (x, y, cw, ch) in enumerate(crops)]).contiguous()

    def dec_b():
        enc.decode_device_crop(crop, results=False)

    def dec_f():
        enc.decode_device_float(full, results=False)

    def dec_c():
        enc.decode_device_crop(crop_all, results=False)
    v = {"a": dec_a, "b": dec_b, "f": dec_f, "c": dec_c}
    for fn in v.values():
        fn()
    torch.cuda.synchronize()
    assert all(s == 0 for d in (full, crop, crop_all) for s in d.statuses())
    ibits = torch.int32 if dtype == torch.float32 else torch.int16
    assert torch.equal(batch.view(ibits), keep["a"].view(ibits)), f"{name}: the crops are not the full decode's slices"
    assert torch.equal(whole2.view(ibits), whole.view(ibits)), f"{name}: the whole-image crop is not the full decode"
    for fn in v.values():
        window(fn, 3)
    t = {key: [] for key in v}
    for _ in range(rounds):
        for key, fn in v.items():
            t[key].append(window(fn, steps))
    med = {key: statistics.median(t[key]) for key in t}
    print(f"{name}, {rounds} rounds x {steps} calls: median ms per call (min-max)", flush=True)
    for key in t:
        print(f"    {key}  {med[key]:8.4f} ms ({min(t[key]):.4f}-{max(t[key]):.4f})", flush=True)
    print(f"    b / a = {med['b'] / med['a']:.3f}   b < a, ranges apart: {'YES' if max(t['b']) < min(t['a']) else 'NO'}", flush=True)
    spread = max(max(t[k]) - min(t[k]) for k in ("f", "c"))
    print(f"    c / f = {med['c'] / med['f']:.3f}   c - f = {med['c'] - med['f']:+.4f} ms, the two's widest min-max range {spread:.4f} ms: "
          f"{'within' if abs(med['c'] - med['f']) <= spread else 'beyond'} the run-to-run spread", flush=True)


def main():
    nums = [a for a in sys.argv[1:] if a.isdigit()]
    names = [a for a in sys.argv[1:] if not a.isdigit()] or list(WORKLOADS)
    rounds, steps = (int(nums[0]) if nums else 7), (int(nums[1]) if len(nums) > 1 else 20)
    assert torch.cuda.is_available(), "this tool measures on a GPU"
    print(f"{torch.cuda.get_device_name(0)}, torch {torch.__version__}, hip {torch.version.hip}", flush=True)
    enc = fpng_amd.Encoder(device=0)
    for key in names:
        workload(enc, *WORKLOADS[key], rounds, steps)
        torch.cuda.empty_cache()
    enc.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
