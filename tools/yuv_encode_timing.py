#!/usr/bin/env python
"""What encoding straight from a video decoder's YUV surfaces costs against what a caller did before it -- torch's chroma
upsample, 3 x 3 multiply-add, round, clamp and to(torch.uint8) into CHW planes, then submit_planar -- on the same box in one process.

    python tools/yuv_encode_timing.py [rounds] [steps]

64 x 1920 x 1080 and 8 x 3840 x 2160 frames, device-resident, flags 0, in NV12 and in P016 (10-bit content in the words' top bits),
BT.709 limited range.  The frames are made of the synthetic "grad" image (Y from its green, Cb / Cr from its blue / red at half
resolution), four distinct frames taking turns.  The variants take turns round by round; a window is `steps` back-to-back calls,
timed on the host clock around a device synchronise; the median window is reported per call with its min-max.  Variants:
  a   submit_yuv on the surfaces (a make_batch_yuv descriptor built once): the fused call
  b   the torch chain into a fresh uint8 NCHW tensor, then submit_planar on it: the yardstick, the path that was there before
  c   submit_planar alone on planes converted beforehand: what the walk costs without any conversion
a's files are checked first, byte for byte, against c's, whose planes are the rule's bytes computed on the host without the library
(tests/yuv_model.py), and counted against b's (torch rounds the products and sums one by one, the rule fuses them: where the two
disagree by a byte the files differ; reported, not asserted).  For a the line also gives the source bytes the call must read over
its time: the achieved load bandwidth of the whole call, not of one kernel."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fpng_amd  # noqa: E402  (before the first torch.cuda call: the library sets the hardware queue count)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import yuv_model  # noqa: E402

DISTINCT = 4


def window(fn, m):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(m):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / m


def host_frames(w, h, sixteen):
    """DISTINCT frames as (Y (h, w), CbCr (h / 2, w / 2, 2)) numpy arrays, uint8 or uint16 with 10 bits in the top of the word"""
    out = []
    for i in range(DISTINCT):
        rgb = fpng_amd.synth_image("grad", w, h, 3, seed=12345 + i)
        y, c = rgb[..., 1].copy(), np.stack([rgb[::2, ::2, 2], rgb[::2, ::2, 0]], axis=-1)
        if sixteen:
            y = (y.astype(np.uint16) << 8) | ((y.astype(np.uint16) * 37) & 0xC0)
            c = (c.astype(np.uint16) << 8) | ((c.astype(np.uint16) * 91) & 0xC0)
        out.append((np.ascontiguousarray(y), np.ascontiguousarray(c)))
    return out


def workload(enc, name, surface, w, h, n, rounds, steps):
    sixteen = surface == "p016"
    m = fpng_amd.yuv_matrix("bt709", False)
    host = host_frames(w, h, sixteen)
    # one surface buffer per frame, as a decoder hands them out: the luma plane, then the chroma plane, one pitch
    elem = 2 if sixteen else 1
    dt = torch.int16 if sixteen else torch.uint8
    surf = torch.empty((n, h + h // 2, w), dtype=dt, device="cuda")
    for i in range(n):
        y, c = host[i % DISTINCT]
        surf[i, :h].copy_(torch.from_numpy(y.view(np.int16) if sixteen else y).cuda())
        surf[i, h:].copy_(torch.from_numpy((c.view(np.int16) if sixteen else c).reshape(h // 2, w)).cuda())
    frames = [(surf[i, :h], surf[i, h:].view(h // 2, w // 2, 2)) for i in range(n)]
    # c's planes: the rule's bytes, made on the host without the library
    pre = torch.empty((n, 3, h, w), dtype=torch.uint8, device="cuda")
    model = [torch.from_numpy(np.ascontiguousarray(yuv_model.to_rgb(surface, f, m).transpose(2, 0, 1))).cuda() for f in host]
    for i in range(n):
        pre[i].copy_(model[i % DISTINCT])
    del model
    cap = fpng_amd.max_encoded_size(w, h, 3) + 64
    outs = {k: [torch.empty(cap, dtype=torch.uint8, device="cuda") for _ in range(n)] for k in "abc"}
    fused = enc.make_batch_yuv(frames, outs["a"], surface=surface, matrix=m)
    planar_c = enc.make_batch_planar(list(pre), outs["c"])
    m_t = torch.from_numpy(m).cuda()
    lum, chroma = surf[:, :h], surf[:, h:].view(n, h // 2, w // 2, 2)
    keep = {}

    def elems(x):
        return (x.to(torch.int32) & 0xFFFF).to(torch.float32) * (1.0 / 256.0) if sixteen else x.to(torch.float32)

    def enc_a():
        enc.submit_yuv(fused)

    def enc_b():
        yf = elems(lum).unsqueeze(1)                                                                       # (n, 1, h, w)
        cf = elems(chroma).repeat_interleave(2, dim=1).repeat_interleave(2, dim=2).permute(0, 3, 1, 2)     # (n, 2, h, w)
        rgb = yf * m_t[:, 0].view(1, 3, 1, 1) + cf[:, 0:1] * m_t[:, 1].view(1, 3, 1, 1) + cf[:, 1:2] * m_t[:, 2].view(1, 3, 1, 1) + m_t[:, 3].view(1, 3, 1, 1)
        keep["q"] = rgb.round().clamp(0, 255).to(torch.uint8)
        enc.submit_planar(list(keep["q"]), outs["b"], 0)

    def enc_c():
        enc.submit_planar(planar_c)
    v = {"a": enc_a, "b": enc_b, "c": enc_c}
    sizes = {}
    for key, fn in v.items():
        fn()
        res = enc.wait(enc.last_ticket, n)
        assert all(st == 0 for _, _, st in res)
        sizes[key] = [s for s, _, _ in res]

    def same(k):
        return sum(sizes["a"][i] == sizes[k][i] and torch.equal(outs["a"][i][:sizes["a"][i]], outs[k][i][:sizes[k][i]]) for i in range(n))
    print(f"{name}, {surface}, flags 0, {rounds} rounds x {steps} calls: median ms per call (min-max)", flush=True)
    print(f"  files identical to those of the rule's bytes (c): {same('c')} of {n}; to the torch chain's (b): {same('b')} of {n}", flush=True)
    assert same("c") == n, f"{name} {surface}: the fused files differ from those of the rule's bytes"
    for fn in v.values():
        window(fn, 3)
    t = {key: [] for key in v}
    for _ in range(rounds):
        for key, fn in v.items():
            t[key].append(window(fn, steps))
    keep.clear()
    med = {key: statistics.median(t[key]) for key in t}
    loaded = n * (h + h // 2) * w * elem
    for key in t:
        extra = f"  {loaded / med[key] / 1e6:7.1f} GB/s of source read" if key == "a" else ""
        print(f"    {key}  {med[key]:8.4f} ms ({min(t[key]):.4f}-{max(t[key]):.4f})  {n * w * h / med[key] / 1e6:7.1f} GP/s{extra}", flush=True)
    apart = max(t["a"]) < min(t["b"])
    print(f"    a / b = {med['a'] / med['b']:.3f}   a / c = {med['a'] / med['c']:.3f}   a < b, ranges apart: {'YES' if apart else 'NO'}", flush=True)
    enc.finish(n)
    return apart


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    enc = fpng_amd.Encoder(device=0)
    ok = True
    for name, w, h, n in (("64 x 1080p", 1920, 1080, 64), ("8 x 3840 x 2160", 3840, 2160, 8)):
        for surface in ("nv12", "p016"):
            ok &= workload(enc, name, surface, w, h, n, rounds, steps)
            torch.cuda.empty_cache()
    enc.close()
    print("fused faster than the torch chain + submit_planar for every surface and workload, ranges apart:", "YES" if ok else "NO")
    return 0


if __name__ == "__main__":
    sys.exit(main())
