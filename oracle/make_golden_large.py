"""Generate tests/golden/large.json from the UNMODIFIED reference (oracle/_ref/libfpng_ref.so): size + sha256 of the files it writes
for images past 2 GiB, or null where it returns false, so that tests/test_gpu_large.py can judge the GPU encoder at the top of the
accepted size range without a CPU encode on the GPU box.

Run in the dev container (where /root/reference exists):   python oracle/make_golden_large.py
One call near 4 GiB takes a few seconds and about 13 GB of host memory (image, the reference's two buffers, the copy out).

  G1  `grad`  24000x24000x4  flags 0, 1, 2   2.3 GB of pixels; compressed IDAT over 2^29 bytes; forced stored over 2^31
  G3  `grad`  30000x24000x3  flags 0         the 3-channel row walk past 2^31 input bytes
  G4  `noise` 28000x28000x4  flags 0         stored fallback: a 3.1 GB file, > 32768 stored blocks, still decodable
  B1  `noise` 63968x16784x4  flags 0, 2      the largest stored outcome the reference writes
  B2  `noise` 63970x16784x4  flags 0, 2      past n*: the reference's 32-bit stored buffer size wraps and it returns false
  B3  `grad`  63970x16784x4  flags 0         B2's shape, compressible

n* = the largest filtered size n = (w*c+1)*h whose stored file the reference writes: 58 + 6 + n + 5*ceil(n/65535) <= 2^32 - 1
(reference src/fpng.cpp:1747, the sum is uint32_t).  Shapes with n in (n*, n* + 64] are avoided: there the wrapped size is below
the 58-byte header and the reference's own buffer arithmetic underflows.
"""
import hashlib
import json
import multiprocessing as mp
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SEED = 12345
CASES = {
    "G1": dict(kind="grad", w=24000, h=24000, c=4, flags=[0, 1, 2]),
    "G3": dict(kind="grad", w=30000, h=24000, c=3, flags=[0]),
    "G4": dict(kind="noise", w=28000, h=28000, c=4, flags=[0]),
    "B1": dict(kind="noise", w=63968, h=16784, c=4, flags=[0, 2]),
    "B2": dict(kind="noise", w=63970, h=16784, c=4, flags=[0, 2]),
    "B3": dict(kind="grad", w=63970, h=16784, c=4, flags=[0]),
}


def one(task):
    name, fl = task
    from cpu_ref import ref
    import fpng_amd
    s = CASES[name]
    img = fpng_amd.synth_image(s["kind"], s["w"], s["h"], s["c"], seed=SEED)
    png = ref().encode(img, s["w"], s["h"], s["c"], fl)
    del img
    if png is None:
        return name, fl, None
    return name, fl, {"size": len(png), "sha256": hashlib.sha256(png).hexdigest(), "idat_len": int.from_bytes(png[50:54], "big")}


def main():
    tasks = [(name, fl) for name, s in CASES.items() for fl in s["flags"]]
    tasks.sort(key=lambda t: -CASES[t[0]]["w"] * CASES[t[0]]["h"])
    with mp.Pool(2) as pool:  # (two at a time: the largest calls hold ~17 GB each)
        res = pool.map(one, tasks, chunksize=1)
    out = {"seed": SEED}
    for name, s in CASES.items():
        e = {k: s[k] for k in ("kind", "w", "h", "c")}
        e["flags"] = {str(fl): r for (nm, fl, r) in res if nm == name}
        out[name] = e
    with open(os.path.join(ROOT, "tests", "golden", "large.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote tests/golden/large.json:", {k: v["flags"] for k, v in out.items() if k != "seed"})


if __name__ == "__main__":
    main()
