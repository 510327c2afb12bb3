"""The rule of fpng_amd_encode_submit_yuv (include/fpng_amd.h, csrc/yuv.h) in numpy, without the library:

    Y = e(luma, x, y);  4:2:0: Cb, Cr = e(chroma, 2 (x >> 1) [+ 1], y >> 1);  4:4:4: Cb = e(plane 1, x, y), Cr = e(plane 2, x, y)
    e(byte) = (float)byte,  e(word) = (float)word * 2^-8
    t_c = fmaf(m[c][2], Cr, fmaf(m[c][1], Cb, fmaf(m[c][0], Y, m[c][3])));   byte_c = rint(min(max(t_c, 0), 255)), ties to even

The chroma indexing is done by slicing (every pixel of a 2 x 2 block takes the block's pair); the arithmetic is
color_model.fma32_np's, exact with one rounding per fmaf, so no element needs a tolerance and ties are fair game.

Also here, for the CPU and the GPU tests alike: the matrix construction of fpng_amd_yuv_matrix recomputed, and surfaces laid out
in one flat byte buffer -- padded pitch, the chroma far away or in front of the luma, planes at odd bytes -- with views of it as
numpy arrays or torch tensors."""
import numpy as np

from color_model import fma32_np

SURFACES = ("nv12", "p016", "yuv444", "yuv444_16")


def is_420(surface):
    return surface in ("nv12", "p016")


def elem_bytes(surface):
    return 2 if surface in ("p016", "yuv444_16") else 1


def elements(plane):
    """e() of a plane: float32, exact (a 16-bit word has 16 significant bits; 2^-8 is a power of two)"""
    p = np.asarray(plane)
    if p.dtype.itemsize == 2:
        return p.view(np.uint16).astype(np.float32) * np.float32(2.0 ** -8)
    return p.astype(np.float32)


def full_chroma(surface, planes):
    """(Cb, Cr), each (h, w) float32: the 4:2:0 pair of a 2 x 2 block given to each of its pixels"""
    h, w = planes[0].shape
    if not is_420(surface):
        return elements(planes[1]), elements(planes[2])
    c = elements(planes[1])  # (ceil(h / 2), ceil(w / 2), 2)
    out = []
    for k in range(2):
        full = np.empty((h, w), dtype=np.float32)
        for i in range(2):
            for j in range(2):
                full[i::2, j::2] = c[:(h - i + 1) // 2, :(w - j + 1) // 2, k]
        out.append(full)
    return out[0], out[1]


def to_rgb(surface, planes, m):
    """(h, w, 3) uint8: the bytes of the file's pixels"""
    m = np.asarray(m, dtype=np.float32)
    y = elements(planes[0])
    cb, cr = full_chroma(surface, planes)
    out = np.empty(y.shape + (3,), dtype=np.uint8)
    for c in range(3):
        t = fma32_np(m[c, 2], cr, fma32_np(m[c, 1], cb, fma32_np(m[c, 0], y, m[c, 3])))
        out[..., c] = np.rint(np.minimum(np.maximum(t, np.float32(0.0)), np.float32(255.0))).astype(np.uint8)
    return out


KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722), "bt2020": (0.2627, 0.0593)}


def matrix(standard, full_range):
    """fpng_amd_yuv_matrix's construction: the nine coefficients in double from Kr and Kb (limited range: luma * 255 / 219, chroma *
    255 / 224), rounded to fp32; then the offsets in double FROM THE ROUNDED coefficients, rounded to fp32"""
    kr, kb = KR_KB[standard]
    kg = 1.0 - kr - kb
    sy, sc, y0 = (1.0, 1.0, 0.0) if full_range else (255.0 / 219.0, 255.0 / 224.0, 16.0)
    coef = [[sy, 0.0, 2.0 * (1.0 - kr) * sc],
            [sy, -(2.0 * kb * (1.0 - kb) / kg) * sc, -(2.0 * kr * (1.0 - kr) / kg) * sc],
            [sy, 2.0 * (1.0 - kb) * sc, 0.0]]
    m = np.zeros((3, 4), dtype=np.float32)
    m[:, :3] = np.asarray(coef, dtype=np.float64).astype(np.float32)
    for c in range(3):
        m[c, 3] = np.float32(-(float(m[c, 0]) * y0 + 128.0 * float(m[c, 1]) + 128.0 * float(m[c, 2])))
    return m


# ---- surfaces in one flat buffer ----
class Layout:
    """Where the planes of a w x h surface lie in a buffer of `total` bytes: the luma's top row at `luma`, rows `pitch` bytes
    apart in every plane, the chroma plane `chroma_offset` bytes from the luma (4:4:4: Cr as far again from Cb).
    place: "tight" (the planes follow each other), "far" (a gap between them), "front" (the chroma in front of the luma: a
    negative offset).  pitch_pad: bytes added to the tight pitch.  start: the first plane's first byte in the buffer (whose
    base is aligned): odd for 8-bit planes at an odd byte, 2 for 16-bit planes at 2 mod 4."""

    def __init__(self, surface, w, h, pitch_pad=0, place="tight", start=0):
        self.surface, self.w, self.h = surface, w, h
        e = self.elem = elem_bytes(surface)
        self.cw = 2 * ((w + 1) // 2) if is_420(surface) else w  # elements of a chroma row
        self.ch = (h + 1) // 2 if is_420(surface) else h
        self.pitch = max(w, self.cw) * e + pitch_pad
        assert self.pitch % e == 0 and start % e == 0
        n_chroma = 1 if is_420(surface) else 2
        luma_bytes, chroma_bytes = h * self.pitch, self.ch * self.pitch
        gap = {"tight": 0, "far": 4096 + 6 * e + (e == 1), "front": 64 + 2 * e + (e == 1)}[place]  # (8-bit: an odd gap)
        if place == "front":
            step = luma_bytes + gap  # from a plane back to the one in front of it (|chroma_offset| is at least the luma plane's span)
            self.luma = start + n_chroma * step
            self.chroma_offset = -step
            self.total = self.luma + luma_bytes + 64
        else:
            self.luma = start
            self.chroma_offset = luma_bytes + gap
            self.total = start + self.chroma_offset * n_chroma + chroma_bytes + 64
        self.total += self.total & 1  # (a whole number of 16-bit words)

    def offsets(self):
        """the byte offset of every plane's top row"""
        n = 2 if is_420(self.surface) else 3
        return [self.luma + k * self.chroma_offset for k in range(n)]

    def plane_shapes(self):
        """per plane (shape, strides in elements)"""
        p = self.pitch // self.elem
        if is_420(self.surface):
            return [((self.h, self.w), (p, 1)), ((self.ch, self.cw // 2, 2), (p, 2, 1))]
        return [((self.h, self.w), (p, 1))] * 3

    def numpy_views(self, buf):
        """the planes as views of the uint8 numpy array buf"""
        dt = np.uint16 if self.elem == 2 else np.uint8
        out = []
        for off, (shape, strides) in zip(self.offsets(), self.plane_shapes()):
            base = buf[off:].view(dt) if (buf.ctypes.data + off) % self.elem == 0 else None
            assert base is not None
            out.append(np.lib.stride_tricks.as_strided(base, shape, tuple(s * self.elem for s in strides)))
        return tuple(out)

    def torch_views(self, buf):
        """the planes as views of the uint8 torch tensor buf (16-bit surfaces: int16 views, which every torch build has)"""
        import torch
        base = buf.view(torch.int16) if self.elem == 2 else buf
        return tuple(torch.as_strided(base, shape, strides, off // self.elem) for off, (shape, strides) in zip(self.offsets(), self.plane_shapes()))


def fill_surface(lay, rng, content="full"):
    """A buffer of random bytes with the surface in it (everything around the planes' pixels stays random).  content: "full" = the
    whole element range; "msb10" = 10-bit values in the words' top bits (P010); "grey" = every chroma element 128 (<< 8)."""
    buf = rng.integers(0, 256, lay.total, dtype=np.uint8)
    planes = lay.numpy_views(buf)
    if content == "msb10":
        for p in planes:
            p &= np.uint16(0xFFC0)
    elif content == "grey":
        for p in planes[1:]:
            p[...] = 128 << (8 if lay.elem == 2 else 0)
    return buf, planes
