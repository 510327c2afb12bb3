"""The rule of fpng_amd_encode_submit_renditions (include/fpng_amd.h) restated in Python without the library, on top of the existing
models, which are imported and not edited: a rendition is img.crop(box).resize(size, filter) -- resize_view_model / resample_model's
passes with `in` = the box's size -- and, for a 4-channel image with alpha "premultiplied", alpha_model's M on load and U on store,
except where Pillow's Image.resize does not premultiply: with the nearest filter, and when size equals the box (self.copy()).
test_renditions_cpu.py pins this text to Pillow and the library's host twin to this text; the GPU tests take their expected pixels
from here."""
import numpy as np

import alpha_model as AM
import resample_model as SM  # noqa: F401  (teaches resize_view_model the four newer filters)
import resize_view_model as VM

FILTERS = ("bilinear", "bicubic", "nearest", "box", "hamming", "lanczos")  # FPNG_AMD_RENDITION_*: their order


def scale_ok(in_size, out_size, filter):
    return SM.scale_ok(in_size, out_size, filter)


def pixels(img, size, box=None, filter="bilinear", alpha=None):
    """img (h, w, c) uint8, R,G,B[,A] -> the rendition's (size[1], size[0], c) uint8 pixels"""
    img = np.asarray(img, dtype=np.uint8)
    x, y, bw, bh = (0, 0, img.shape[1], img.shape[0]) if box is None else box
    planes = np.ascontiguousarray(img[y:y + bh, x:x + bw].transpose(2, 0, 1))
    size = (int(size[0]), int(size[1]))
    if planes.shape[0] == 4 and alpha == "premultiplied" and filter != "nearest" and size != (bw, bh):
        r = AM.view_planes({"op": "premultiplied"}, planes, size, None, filter)
    else:
        r = VM.view_planes(planes, size, None, filter)
    return np.ascontiguousarray(r.transpose(1, 2, 0))
