#!/usr/bin/env python
"""What the per-view RESAMPLE record of the views call (fpng_amd_decode_batch_device_planar_views_resample) costs: one device-resident
call of 64 three-channel 1080p files x 2 RandomResizedCrop views of 224 x 224 into an f16 batch with ImageNet's constants, every
second view mirrored (a sibling of tools/views_alpha_timing.py, whose crops, window and rounds it uses).

    python tools/views_resample_timing.py [rounds] [steps] [files]

  alpha      the views call with alpha= records without an op: what a tree without the record runs (run it there for the parent's
             number; the other sides are then left out)
  resample0  resample= with records without a filter: the same kernels as `alpha`
  bicubic    filter="bicubic", no record
  nearest, box, hamming, lanczos   the four RESAMPLE filters, every view of the call
The sides take turns round by round; a window is `steps` back-to-back calls between two device events, after a warm-up of all; the
median window per call with its min-max over the rounds."""
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
from views_timing import random_resized_crop  # noqa: E402

SIDE = 224


def main():
    nums = [int(a) for a in sys.argv[1:] if a.isdigit()]
    rounds, steps, n = (nums + [9, 50, 64][len(nums):])[:3]
    assert torch.cuda.is_available(), "this tool measures on a GPU"
    enc = fpng_amd.Encoder(device=0)
    dev = files_on_device(enc, W, H, n)
    rng = np.random.default_rng(2024)
    crops = [[random_resized_crop(rng, (0.08, 1.0)) for _ in range(2)] for _ in range(n)]
    mirrors = [[False, True] for _ in range(n)]
    x = torch.empty((n * 2, 3, SIDE, SIDE), dtype=torch.float16, device="cuda")
    outs = [[x[2 * i], x[2 * i + 1]] for i in range(n)]

    def descriptor(**kw):
        return enc.make_decode_batch_views(dev, crops, outs, (SIDE, SIDE), mirror=mirrors, mean=MEAN, std=STD, **kw)

    db = {"alpha": descriptor(alpha=fpng_amd.view_alpha())}
    if hasattr(fpng_amd, "view_resample"):
        db["resample0"] = descriptor(resample=fpng_amd.view_resample())
        db["bicubic"] = descriptor(filter="bicubic")
        for f in ("nearest", "box", "hamming", "lanczos"):
            db[f] = descriptor(resample=f)
    fns = {k: (lambda d=d: enc.decode_device_views(d, results=False)) for k, d in db.items()}
    for k, fn in fns.items():
        window(fn, 3)
        assert list(db[k].statuses()) == [0] * n, k
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            t[k].append(window(fn, steps))
    print(f"{torch.cuda.get_device_name(0)}, torch {torch.__version__}: {n} device-resident {W} x {H} RGB files x 2 views of {SIDE} x {SIDE} -> f16; {rounds} rounds of {steps} calls; "
          "ms per call, median (min-max)")
    for k, v in t.items():
        print(f"  {k:10s} {statistics.median(v):.4f} ({min(v):.4f}-{max(v):.4f})")
    enc.close()


if __name__ == "__main__":
    main()
