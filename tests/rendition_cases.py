"""Sources for the rendition tests in the layouts of the four descriptor kinds, as torch tensor VIEWS over a flat buffer whose other
bytes (pitch padding, X bytes, a foreign plane) come from `fill` -- on the host for test_renditions_cpu.py (the twin reads them),
on the GPU for test_gpu_renditions.py."""
import numpy as np
import torch

from test_gpu_layouts import _layout, _to_source


def ex_view(img, name, pitch_kind, fill, device="cpu"):
    """img (h, w, c) R,G,B[,A] as FPNG_AMD_SRC_<name> pixels laid out by test_gpu_layouts._layout (packed | odd | wide | neg) ->
    (buffer tensor, its host copy, the (h, w, c) view submit_ex takes, order, bottom_up)"""
    src = _to_source(img, name, fill)
    h, w, sb = src.shape
    buf, top, pitch = _layout(src, pitch_kind, fill)
    d = torch.from_numpy(buf).to(device)
    first = top if pitch > 0 else top + (h - 1) * pitch  # the lowest row's first byte
    full = torch.as_strided(d, (h, w, sb), (abs(pitch), sb, 1), first)
    if name[0] == "X":
        view, order = full[..., 1:], name[1:].lower()
    elif name[-1] == "X":
        view, order = full[..., :3], name[:3].lower()
    else:
        view, order = full, name.lower()
    return d, buf, view, order, pitch < 0


def planar_view(img, reverse, fill, device="cpu", pad=5):
    """img (h, w, c) as planes of a (4, h + 2, w + pad) uint8 tensor (a 3-channel image: the plane behind or in front of its three is
    the caller's), rows padded; reverse: the planes stored [A,] B, G, R (a negative plane pitch) -> (buffer tensor, host copy, the
    (c, h, w) view, order)"""
    h, w, c = img.shape
    host = fill.integers(0, 256, (4, h + 2, w + pad), dtype=np.uint8) if fill is not None else np.zeros((4, h + 2, w + pad), dtype=np.uint8)
    planes = img.transpose(2, 0, 1)
    first = 4 - c if reverse else 0  # (reversed planes end at the buffer's last plane: the foreign one lies in front)
    host[first:first + c, 1:h + 1, 2:w + 2] = planes[::-1] if reverse else planes
    d = torch.from_numpy(host).to(device)
    return d, host, d[first:first + c, 1:h + 1, 2:w + 2], ("abgr" if c == 4 else "bgr") if reverse else "rgb"


def float_tensor(el, code, device="cpu"):
    """elements (h, w, c) as test_float_encode_cpu makes them (code 2: bf16 bits in uint16) -> the contiguous (c, h, w) tensor"""
    chw = np.ascontiguousarray(el.transpose(2, 0, 1))
    t = torch.from_numpy(chw.view(np.int16)).view(torch.bfloat16) if code == 2 else torch.from_numpy(chw)
    return t.to(device)
