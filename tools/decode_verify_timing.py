#!/usr/bin/env python
"""What checking the checksums costs the GPU decoder (fpng_amd_encoder_set_decode_verify), and that the default path costs what it did.

    python tools/decode_verify_timing.py [--reps 6] [--runs 5] [--only TEXT] [--verify 0,1,2,3] [--no-host] [--parent]

Per case -- n device-resident files decoded where they lie (fpng_amd_decode_batch_device), and fpng_amd_decode_host on one 8K file
-- and per verify value 0, 1 (CRC-32), 2 (Adler-32), 3: `runs` runs of `reps` calls each, a run's figure being its best call's wall
time (host parse + kernels + status read-back); printed are the runs' minimum, median and maximum, i.e. the spread that a
difference has to be held against.  --parent: the library (FPNG_AMD_LIB=<an older build's libfpng_amd.so>) has no verify calls:
verify 0 only, for the same-box comparison of the default path."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=6)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--only", default="")
ap.add_argument("--parent", action="store_true")
ap.add_argument("--verify", default="0,1,2,3", help="the verify values to time, verify 0 first when it is among them")
ap.add_argument("--no-host", action="store_true", help="leave out fpng_amd_decode_host")
args = ap.parse_args()
import warnings
with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    from fpng_amd import _lib
if args.parent:
    for name in ("fpng_amd_encoder_set_decode_verify", "fpng_amd_encoder_decode_verify"):
        _lib.SIGNATURES.pop(name, None)
import numpy as np, torch, fpng_amd  # noqa: E401,E402

enc = fpng_amd.Encoder(device=0)
levels = (0,) if args.parent else tuple(int(v) for v in args.verify.split(","))
print(f"library: {_lib.LIB_PATH}; {args.runs} runs of {args.reps} calls, ms: min / median / max of the runs' best calls", flush=True)


def runs_of(call):
    out = []
    for _ in range(args.runs):
        best = 1e9
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            best = min(best, time.perf_counter() - t0)
        out.append(best * 1e3)
    return out


def report(name, level, ms, base):
    extra = "" if base is None else f"  (+{min(ms) - base:6.3f} ms against verify 0)"
    print(f"{name:28s} verify {level}: {min(ms):8.3f} / {statistics.median(ms):8.3f} / {max(ms):8.3f}{extra}", flush=True)


# (name, [(kind, w, h, c, n), ...]): the last case is one large file among many small ones -- the CRC pass and the stored files' Adler
# pass size their grids by the batch's largest file, so every small file launches that many workgroups, which leave at once
cases = [("8K RGBA grad x 8", [("grad", 7680, 4320, 4, 8)]), ("8K RGBA noise x 8 (stored)", [("noise", 7680, 4320, 4, 8)]),
         ("1080p RGB grad x 64", [("grad", 1920, 1080, 3, 64)]), ("512x512 RGB grad x 256", [("grad", 512, 512, 3, 256)]),
         ("mixed: 8K noise x 1 + 512x512 x 255, RGBA", [("noise", 7680, 4320, 4, 1), ("grad", 512, 512, 4, 255)])]
for name, parts in cases:
    if args.only and args.only not in name:
        continue
    c = parts[0][3]
    ts = [torch.from_numpy(fpng_amd.synth_image(kind, w, h, c, seed=12345 + i)).cuda() for kind, w, h, c, n in parts for i in range(n)]
    dims = [(w, h) for kind, w, h, c, n in parts for i in range(n)]
    pngs = []
    for k in range(0, len(ts), 64):
        pngs += enc.encode_tensors(ts[k:k + 64], 0)[0]
    dev = [torch.frombuffer(bytearray(p), dtype=torch.uint8).cuda() for p in pngs]
    outs = [torch.empty(w * h * c, dtype=torch.uint8, device="cuda") for w, h in dims]
    db = enc.make_decode_batch(dev, c, dims, outs)
    base = None
    for level in levels:
        if not args.parent:
            enc.set_decode_verify(level)
        ms = runs_of(lambda: enc.decode_device(db, results=False))
        got = db.results()
        assert all(st == 0 for st, _, _ in got), [st for st, _, _ in got]
        assert all(torch.equal(px.reshape(-1), t.reshape(-1)) for (st, px, _), t in zip(got, ts))
        report(name + f" [{sum(len(p) for p in pngs) / 1e6:.0f} MB]", level, ms, base if level else None)
        base = min(ms) if base is None else base
    del ts, dev, outs, db
    torch.cuda.empty_cache()

if not args.no_host and (not args.only or args.only in "host call 8K RGBA grad"):
    w, h, c = 7680, 4320, 4
    img = fpng_amd.synth_image("grad", w, h, c, seed=12345)
    (png,), _ = enc.encode_tensors([torch.from_numpy(img).cuda()], 0)
    png = bytes(png)
    base = None
    for level in levels:
        if not args.parent:
            enc.set_decode_verify(level)
        res = []
        ms = runs_of(lambda: res.__setitem__(slice(None), [enc.decode_host(png, c)]))
        st, px, _ = res[0]
        assert st == 0 and np.array_equal(px.reshape(-1), img.reshape(-1))
        report("host call 8K RGBA grad", level, ms, base if level else None)
        base = min(ms) if base is None else base
if not args.parent:
    enc.set_decode_verify(0)
enc.close()
