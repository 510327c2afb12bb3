#!/usr/bin/env python
"""GPU decode of DEVICE-resident files into NV12 surfaces (fpng_amd_decode_batch_device_yuv_views), timed with events on the
encoder's stream, best of `reps` steps of 8 x 4K RGB files:
  1. -> NV12 at 1080p (one resized view per file);
  2. -> NV12 at the files' own size (the identity view);
  3. what a caller did before the call existed: decode_device_views() into uint8 planes at the same size, then a torch expression
     of the same conversion as a second step.
(profiles/yuv_store_timing.txt)"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch, fpng_amd
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 8
n, w, h = 8, 3840, 2160
enc = fpng_amd.Encoder(device=0)
ts = [torch.from_numpy(fpng_amd.synth_image("grad", w, h, 3, seed=12345 + i)).cuda() for i in range(n)]
pngs, _ = enc.encode_tensors(ts, 0)
dev = [torch.frombuffer(bytearray(p), dtype=torch.uint8).cuda() for p in pngs]
m = torch.from_numpy(fpng_amd.yuv_matrix_from_rgb("bt709", False)).cuda()


def timed(step):
    best = 1e9
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(); a.record(); step(); b.record(); torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b))
    return best


def torch_nv12(planes):
    """(3, h, w) uint8 planes (even sizes) -> Y (h, w), CbCr (h / 2, w / 2, 2): the rule's conversion without its fused roundings"""
    p = planes.float()
    mix = lambda c, q: (m[c, 0] * q[0] + m[c, 1] * q[1] + m[c, 2] * q[2] + m[c, 3]).clamp_(0, 255).round_().to(torch.uint8)
    q = torch.nn.functional.avg_pool2d(p[None], 2)[0]
    return mix(0, p), torch.stack([mix(1, q), mix(2, q)], dim=-1)


for name, (ow, oh) in (("1080p", (1920, 1080)), ("native 2160p", (w, h))):
    crops, fulls = [[(0, 0, w, h)]] * n, [[(ow, oh)]] * n
    yuv = enc.decode_device_yuv(dev, None, "nv12", crops=crops, full=fulls, results=False)
    t_yuv = timed(lambda: enc.decode_device_yuv(yuv, results=False))
    assert all(st == 0 for st, _, _ in yuv.results())
    planar = enc.decode_device_views(dev, crops, None, fulls, results=False)
    t_views = timed(lambda: enc.decode_device_views(planar, results=False))
    outs = [ts_[0] for _, ts_, _ in planar.results()]
    t_both = timed(lambda: (enc.decode_device_views(planar, results=False), [torch_nv12(t) for t in outs]))
    # the two roads agree to the rounding of the unfused expression
    ya, yb = yuv.results()[0][1][0][0], torch_nv12(outs[0])[0]
    assert int((ya.int() - yb.int()).abs().max()) <= 1
    print(f"8 x 4K RGB grad -> NV12 {name}: decode_device_yuv {t_yuv:7.3f} ms; decode_device_views (uint8 planes) {t_views:7.3f} ms; "
          f"decode_device_views + torch conversion {t_both:7.3f} ms", flush=True)
