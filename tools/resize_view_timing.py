#!/usr/bin/env python
"""Two measurements around fpng_amd_decode_batch_device_planar_resize_view, on one box in one process each (a sibling of
tools/resize_decode_timing.py, whose windows and rounds it uses).

    python tools/resize_view_timing.py old  [rounds] [steps] [files]
    python tools/resize_view_timing.py eval [rounds] [steps] [files]

old   The plain resize call, which now runs through the view path: 256 device-resident 1080p RGB files, seeded RandomResizedCrop
      boxes -> one (n, 3, 224, 224) f16 batch with ImageNet's mean / std through decode_device_resize (resize_decode_timing's
      variant b, same seeds).  Prints the median window per call and its min-max over the rounds.  To compare two builds, run it
      from each build's tree in turn, several times over (the library is chosen when the process starts): the margin is the
      earlier build's own round-to-round range.
eval  The evaluation transform Resize(256) + CenterCrop(224) + Normalize -> f16 of 256 device-resident 500 x 375 RGB files (four
      distinct `grad` images, repeated).  The variants take turns round by round:
        a-bilinear / a-bicubic   what there was before: decode_device into uint8 HWC tensors, then per file
                                 F.interpolate(antialias=True) to 341 x 256, the centre slice, normalise, a copy into the batch
        b-bilinear / b-bicubic   decode_device_resize_view into the views of the batch
        c                        decode_device_crop of the bicubic views' source boxes to uint8 alone (b's first stage)
      b is checked against a first: the resamplers differ (a: float, torch's; b: Pillow's 8-bit rule), so the check is a mean
      absolute difference below one byte step -- a gross error (wrong window) fails it.  The resize stage's share: the encoder's
      profiling events bracket the kernels behind the synchronisation -- b's bracket minus c's is the resize stage."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fpng_amd  # noqa: E402  (before the first torch.cuda call: the library sets the hardware queue count)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from resize_decode_timing import MEAN, STD, random_resized_crop, window  # noqa: E402

SIDE = 224


def files_on_device(enc, w, h, n):
    pngs = []
    for i in range(4):
        (p,), _ = enc.encode_tensors([torch.from_numpy(fpng_amd.synth_image("grad", w, h, 3, seed=12345 + i)).cuda()], 0)
        pngs.append(p)
    return [torch.frombuffer(bytearray(pngs[i % 4]), dtype=torch.uint8).cuda() for i in range(n)]


def rounds_of(v, rounds, steps):
    for fn in v.values():
        window(fn, 3)
    t = {key: [] for key in v}
    for _ in range(rounds):
        for key, fn in v.items():
            t[key].append(window(fn, steps))
    return t


def old(rounds, steps, n):
    enc = fpng_amd.Encoder(device=0)
    dev = files_on_device(enc, 1920, 1080, n)
    rng = np.random.default_rng(2024)
    crops = [random_resized_crop(rng) for _ in range(n)]
    batch = torch.empty((n, 3, SIDE, SIDE), dtype=torch.float16, device="cuda")
    db = enc.make_decode_batch_resize(dev, crops, list(batch), mirror=[bool(i & 1) for i in range(n)], mean=MEAN, std=STD)

    def dec():
        enc.decode_device_resize(db, results=False)
    dec()
    torch.cuda.synchronize()
    assert all(s == 0 for s in db.statuses())
    t = rounds_of({"b": dec}, rounds, steps)["b"]
    print(f"old call, {n} x 1080p RGB -> {SIDE}x{SIDE} f16, {rounds} rounds x {steps} calls, library {os.path.relpath(fpng_amd._lib.LIB_PATH, ROOT)}: "
          f"median {statistics.median(t):.4f} ms per call ({min(t):.4f}-{max(t):.4f}); sum of the batch's bits {int(batch.view(torch.int16).long().sum())}", flush=True)
    enc.close()


def evaluation(rounds, steps, n):
    w, h = 500, 375
    enc = fpng_amd.Encoder(device=0)
    dev = files_on_device(enc, w, h, n)
    crop, full, win = fpng_amd.center_crop_view(w, h, 256, SIDE)
    x0, y0 = win[0], win[1]
    whole = [torch.empty((h, w, 3), dtype=torch.uint8, device="cuda") for _ in range(n)]
    full_db = enc.make_decode_batch(dev, 3, [(w, h)] * n, [t.view(-1) for t in whole])
    mean = torch.tensor(MEAN, device="cuda")[:, None, None]
    std = torch.tensor(STD, device="cuda")[:, None, None]
    batches = {key: torch.empty((n, 3, SIDE, SIDE), dtype=torch.float16, device="cuda") for key in ("a-bilinear", "a-bicubic", "b-bilinear", "b-bicubic")}
    views = {f: enc.make_decode_batch_resize_view(dev, [crop] * n, list(batches["b-" + f]), full, win, f, mean=MEAN, std=STD) for f in ("bilinear", "bicubic")}
    box = fpng_amd.resize_view_source(crop, full, win, "bicubic")
    boxes = [torch.empty((3, box[3], box[2]), dtype=torch.uint8, device="cuda") for _ in range(n)]
    box_db = enc.make_decode_batch_crop(dev, [box] * n, boxes)

    def dec_a(mode):
        out = batches["a-" + mode]

        def run():
            enc.decode_device(full_db, results=False)
            for i, t in enumerate(whole):
                x = F.interpolate(t.permute(2, 0, 1)[None].float(), size=(full[1], full[0]), mode=mode, antialias=True)[0]
                out[i] = (x[:, y0:y0 + SIDE, x0:x0 + SIDE] / 255.0 - mean) / std
        return run

    v = {"a-bilinear": dec_a("bilinear"), "a-bicubic": dec_a("bicubic"),
         "b-bilinear": lambda: enc.decode_device_resize_view(views["bilinear"], results=False),
         "b-bicubic": lambda: enc.decode_device_resize_view(views["bicubic"], results=False),
         "c": lambda: enc.decode_device_crop(box_db, results=False)}
    for fn in v.values():
        fn()
    torch.cuda.synchronize()
    assert all(s == 0 for d in (views["bilinear"], views["bicubic"], box_db) for s in d.statuses())
    step = 1.0 / 255.0 / min(STD)
    for f in ("bilinear", "bicubic"):
        diff = (batches["a-" + f].float() - batches["b-" + f].float()).abs()
        print(f"b-{f} against a-{f}: mean |difference| {float(diff.mean()):.5f}, max {float(diff.max()):.5f} (one byte step: {step:.5f})", flush=True)
        assert float(diff.mean()) < step, "the new call's batch is not the baseline's"
    t = rounds_of(v, rounds, steps)
    med = {key: statistics.median(t[key]) for key in t}
    print(f"{n} x {w}x{h} RGB, Resize(256) + CenterCrop({SIDE}) + Normalize -> f16 (full {full[0]}x{full[1]}, window {win}, bicubic source box {box}), "
          f"{rounds} rounds x {steps} calls: median ms per call (min-max)", flush=True)
    for key in t:
        print(f"    {key:11s} {med[key]:8.4f} ms ({min(t[key]):.4f}-{max(t[key]):.4f})", flush=True)
    for f in ("bilinear", "bicubic"):
        print(f"    b-{f} / a-{f} = {med['b-' + f] / med['a-' + f]:.3f}", flush=True)
    enc.set_profiling(True)
    ph = {"b-bilinear": [], "b-bicubic": [], "c": []}
    for _ in range(rounds):
        for key in ph:
            v[key]()
            torch.cuda.synchronize()
            ph[key].append(enc.last_decode_phase_ms()["unfilter"])
    enc.set_profiling(False)
    pm = {key: statistics.median(ph[key]) for key in ph}
    for key in ph:
        print(f"    kernels behind the synchronisation, {key:11s} {pm[key]:.4f} ms ({min(ph[key]):.4f}-{max(ph[key]):.4f})", flush=True)
    for f in ("bilinear", "bicubic"):
        stage = pm["b-" + f] - pm["c"]
        print(f"    the resize stage, {f} (b - c): {stage:.4f} ms for {n} files x 3 planes, {100 * stage / med['b-' + f]:.0f} % of the call", flush=True)
    enc.close()


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode not in ("old", "eval"):
        print(__doc__)
        return 2
    nums = [int(a) for a in sys.argv[2:] if a.isdigit()]
    rounds, steps, n = (nums + [7, 10, 256][len(nums):])[:3]
    assert torch.cuda.is_available(), "this tool measures on a GPU"
    print(f"{torch.cuda.get_device_name(0)}, torch {torch.__version__}, hip {torch.version.hip}", flush=True)
    (old if mode == "old" else evaluation)(rounds, steps, n)
    return 0


if __name__ == "__main__":
    sys.exit(main())
