#!/usr/bin/env python
"""What eight 1920 x 1080 bilinear renditions of eight device-resident 8K RGBA frames cost per submission, next to what a caller
did before there was fpng_amd_encode_submit_renditions.  Not a test and not part of bench.py.

    python tools/rendition_timing.py --form new|a|b [--steps K] [--repeats R] [--package-root DIR]

Three forms, one per process:
  new  Encoder.submit_renditions(): 8 x (4320, 7680, 4) uint8 -> eight 1920 x 1080 bilinear renditions, one submission
  a    the floor: Encoder.submit() of eight ready-made 1080p RGBA images (no resize at all)
  b    what a caller did: per frame F.interpolate(..., mode="bilinear", antialias=True) of the float NCHW view, round, clamp, to
       uint8, a permute copy back to HWC, then Encoder.submit() of the eight results
Forms a and b use nothing of this commit, so --package-root <a checkout of the parent commit with its library built> times them on
the parent's build on the same machine (the parent's package has no form "new").

A repeat is K submissions made back to back with at most three in flight (the settled state of a pipeline: lanes busy, scratch
grown, code loaded), ended by a device synchronise; its time is the host clock over K, and K defaults to what makes a repeat last
about half a second.  Two warm-up repeats, then R timed ones: the median with its min-max, which is the spread any comparison has
to be read against.  Compare forms within one session, alternating them (new, a, b, new, a, b, ...).  The resize kernel's own time is not
taken here: a kernel trace (rocprofv3 --kernel-trace --stats -- python tools/rendition_timing.py --form new --repeats 1) has it as
enc_resize_kernel.  Form b's bytes are NOT the rendition's (float arithmetic against Pillow's fixed point): the forms are compared
for time only."""
import argparse
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--form", required=True, choices=["new", "a", "b"])
ap.add_argument("--steps", type=int, default=None, help="submissions per repeat; default: about half a second per repeat (new 600, a 8000, b 48)")
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
args = ap.parse_args()
if args.steps is None:
    args.steps = {"new": 600, "a": 8000, "b": 48}[args.form]
sys.path.insert(0, os.path.abspath(args.package_root))
import fpng_amd  # noqa: E402  (before the first torch.cuda call: the library sets the hardware queue count)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

N, SRC_W, SRC_H, W, H, C = 8, 7680, 4320, 1920, 1080, 4


def main():
    assert torch.cuda.is_available(), "rendition_timing.py measures on a GPU and nowhere else"
    enc = fpng_amd.Encoder(device=0)
    print(f"library: {fpng_amd._lib.LIB_PATH}   lanes {enc.lanes}   form {args.form}", flush=True)
    outs = [[torch.empty(fpng_amd.max_encoded_size(W, H, C) + 64, dtype=torch.uint8, device="cuda") for _ in range(N)] for _ in range(4)]
    if args.form == "a":
        small = [torch.from_numpy(fpng_amd.synth_image("blocks" if i & 1 else "grad", W, H, C, seed=12345 + i)).cuda() for i in range(N)]
    else:
        frames = [torch.from_numpy(fpng_amd.synth_image("blocks" if i & 1 else "grad", SRC_W, SRC_H, C, seed=12345 + i)).cuda() for i in range(N)]
    if args.form == "new":
        rends = [fpng_amd.rendition(i, (W, H), filter="bilinear") for i in range(N)]

    def step(k):
        o = outs[k % 4]
        if args.form == "new":
            enc.submit_renditions(frames, rends, outs=o)
        elif args.form == "a":
            enc.submit(small, o)
        else:
            made = []
            for f in frames:
                y = F.interpolate(f.permute(2, 0, 1)[None].float(), size=(H, W), mode="bilinear", antialias=True)
                made.append(y.round_().clamp_(0, 255).to(torch.uint8)[0].permute(1, 2, 0).contiguous())
            enc.submit(made, o)
        return enc.last_ticket

    def repeat():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tickets = []
        for k in range(args.steps):
            tickets.append(step(k))
            if k >= 3:
                enc.wait(tickets[k - 3], N)
        res = enc.finish(N)
        torch.cuda.synchronize()
        assert all(st == 0 for _, _, st in res)
        return (time.perf_counter() - t0) * 1e3 / args.steps, sum(s for s, _, _ in res)

    for _ in range(2):
        _, size = repeat()
    ms = [repeat()[0] for _ in range(args.repeats)]
    print(f"form {args.form}: {N} x {'1080p RGBA ready-made' if args.form == 'a' else '8K RGBA -> 1920 x 1080'}, 1-pass, {args.steps} submissions per repeat, "
          f"{args.repeats} repeats: {statistics.median(ms):.3f} ms per submission (min-max {min(ms):.3f}-{max(ms):.3f}); the eight files {size / 1e6:.2f} MB", flush=True)
    enc.close()


if __name__ == "__main__":
    main()
