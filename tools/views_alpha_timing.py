#!/usr/bin/env python
"""What the per-view alpha record of the views call (fpng_amd_decode_batch_device_planar_views_alpha) costs: one device-resident call
of 64 four-channel 1080p files x 2 RandomResizedCrop views of 224 x 224 into an f16 batch of three planes with ImageNet's constants,
every second view mirrored (a sibling of tools/views_warp_timing.py, whose crops, window and rounds it uses).  The files are a
gradient under an alpha plane that is 0 in a frame, 255 in the middle and a ramp between the two.

    python tools/views_alpha_timing.py [rounds] [steps] [files]

  enhance        the views call with enhance= records without an op: what a tree without the stage runs (run it there for the
                 parent's number; the other sides are then left out)
  op0            alpha= with records without an op: the same kernels as `enhance`
  composite      every view over its own background colour
  premultiplied  every view resized premultiplied
  rgba           the caller-side alternative to `composite`: four planes out of the views call...
  rgba+torch     ...and then the composite over the same backgrounds in torch -- in floats, behind the resize: not the same values,
                 the same work
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
from views_timing import random_resized_crop  # noqa: E402

SIDE = 224


def rgba_files_on_device(enc, n):
    """four distinct files, repeated: a gradient whose alpha is 0 in a frame of an eighth of the size, 255 in the middle half and a
    linear ramp between them"""
    x, y = np.arange(W, dtype=np.float64)[None, :], np.arange(H, dtype=np.float64)[:, None]
    edge = np.minimum(np.minimum(x, W - 1 - x) / W, np.minimum(y, H - 1 - y) / H)  # 0 at the border .. 0.5
    alpha = np.clip((edge - 0.125) / 0.125, 0.0, 1.0)
    pngs = []
    for i in range(4):
        img = fpng_amd.synth_image("grad", W, H, 4, seed=12345 + i).copy()
        img[..., 3] = np.rint(255.0 * alpha).astype(np.uint8)
        (p,), _ = enc.encode_tensors([torch.from_numpy(img).cuda()], 0)
        pngs.append(p)
    return [torch.frombuffer(bytearray(pngs[i % 4]), dtype=torch.uint8).cuda() for i in range(n)]


def main():
    nums = [int(a) for a in sys.argv[1:] if a.isdigit()]
    rounds, steps, n = (nums + [9, 50, 64][len(nums):])[:3]
    assert torch.cuda.is_available(), "this tool measures on a GPU"
    enc = fpng_amd.Encoder(device=0)
    dev = rgba_files_on_device(enc, n)
    rng = np.random.default_rng(2024)
    crops = [[random_resized_crop(rng, (0.08, 1.0)) for _ in range(2)] for _ in range(n)]
    mirrors = [[False, True] for _ in range(n)]
    bgs = [[tuple(int(v) for v in rng.integers(0, 256, 3)) for _ in range(2)] for _ in range(n)]
    x3 = torch.empty((n * 2, 3, SIDE, SIDE), dtype=torch.float16, device="cuda")
    x4 = torch.empty((n * 2, 4, SIDE, SIDE), dtype=torch.float16, device="cuda")
    outs3, outs4 = [[x3[2 * i], x3[2 * i + 1]] for i in range(n)], [[x4[2 * i], x4[2 * i + 1]] for i in range(n)]

    def descriptor(outs, mean, std, **kw):
        return enc.make_decode_batch_views(dev, crops, outs, (SIDE, SIDE), mirror=mirrors, mean=mean, std=std, **kw)

    db = {"enhance": descriptor(outs3, MEAN, STD, enhance=fpng_amd.view_enhance())}
    if hasattr(fpng_amd, "view_alpha"):
        db["op0"] = descriptor(outs3, MEAN, STD, alpha=fpng_amd.view_alpha())
        db["composite"] = descriptor(outs3, MEAN, STD, alpha=[[fpng_amd.view_alpha("composite", b) for b in row] for row in bgs])
        db["premultiplied"] = descriptor(outs3, MEAN, STD, alpha=fpng_amd.view_alpha("premultiplied"))
    # (the caller's own composite: plain [0, 1] planes out, v * a + b * (1 - a), then the normalisation)
    db["rgba"] = descriptor(outs4, (0.0,) * 4, (1.0,) * 4)
    fns = {k: (lambda d=d: enc.decode_device_views(d, results=False)) for k, d in db.items()}
    bg = torch.tensor([b for row in bgs for b in row], dtype=torch.float16, device="cuda").div_(255.0).reshape(n * 2, 3, 1, 1)
    mean, std = (torch.tensor(v, dtype=torch.float16, device="cuda").reshape(1, 3, 1, 1) for v in (MEAN, STD))

    def rgba_torch():
        fns["rgba"]()
        a = x4[:, 3:4]
        return (x4[:, :3] * a + bg * (1 - a)).sub_(mean).div_(std)

    fns["rgba+torch"] = rgba_torch
    for k, fn in fns.items():
        window(fn, 3)
        assert k not in db or list(db[k].statuses()) == [0] * n, k
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            t[k].append(window(fn, steps))
    print(f"{torch.cuda.get_device_name(0)}, torch {torch.__version__}: {n} device-resident {W} x {H} RGBA files x 2 views of {SIDE} x {SIDE} -> f16; {rounds} rounds of {steps} calls; "
          "ms per call, median (min-max)")
    for k, v in t.items():
        print(f"  {k:14s} {statistics.median(v):.4f} ({min(v):.4f}-{max(v):.4f})")
    enc.close()


if __name__ == "__main__":
    main()
