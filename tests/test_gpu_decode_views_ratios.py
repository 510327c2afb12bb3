"""The DEVICE compile of the resize's weight text over a sweep of scale ratios (-m gpu).  resize.h promises that the kernels and the host
twins compile ONE text -- resample_weights_of, resample_taps, resize_sin, resize_cos, the truncations of center -/+ support + 0.5 --
and agree bit for bit; the host compile is swept over some 13 000 size pairs per filter against Pillow
(test_views_resample_cpu.py), the device compile used to meet the fifteen-odd ratios of the views tests' shapes.  Here every (in, out)
pair of ratio_sweep.py inside the filter's limit -- 1550 to 1702 per filter -- is an axis of a view of ONE 3-channel 128 x 128 file,
once as the view's x axis and once as its y axis, and all of a filter's views are decoded in ONE call (the file is decoded once; no
call has refused that many views): planar destinations run dec_resize_exact_kernel, channels-last ones dec_resize_hwc_kernel.
Bilinear and bicubic run twice: without resample= (launch kinds 0 and 1), and with one NEAREST view added to the call (kind 2, where
resample_weights_of forwards to resize_weights_of); the two buffers must be equal on the shared views.

What the sweep pins and what it cannot (test_views_ratio_sweep_cpu.py has the figures): a first tap or a count that rounds
differently on the device changes bytes under box, whose weights do not vanish at the support's edge, and an index table that
differs changes bytes under nearest -- mutants of the model that do either, or close the box interval on the other side, change
hundreds of the sweep's views.  Under Hamming, Lanczos, bilinear and bicubic a tap that moves at the support's edge carries a
weight of about zero and changes no byte, and a weight off by one unit of 2^-22 reaches a byte in about 6 of 10^5 samples: the
sweep does not pin every weight's last bit.  It pins the BYTES, for all six filters; the bytes are the contract.

The image is noise whose even columns and even rows are 0 or 255, so that the sums of both passes reach both clips.  Expected values
never come from the library: the planes are the REFERENCE's decoder's, resized by resample_model.py / resize_view_model.py and
turned into elements by alpha_model.view_elements; a filter's expected views are computed once (about 2 s) and shared by the two
layouts.  Every call decodes into ONE sentinel-filled buffer that is compared WHOLE and bit for bit."""
import numpy as np
import pytest

from test_gpu_decode_float import CONSTS
from test_gpu_decode_layouts import _encode_gpu
from test_gpu_decode_resize import _Files, enc  # noqa: F401  (enc: a fixture)
from test_gpu_decode_views_color import LAYOUTS, _difference
from test_gpu_decode_views_resample_alpha import _decode, _kinds
import ratio_sweep as RS  # (imports resample_model before any model is asked for a new filter's name)
import alpha_model as AM
import resize_view_model as VM

pytestmark = pytest.mark.gpu

NEAREST_VIEW = ((3, 5, 64, 40), (24, 33), True)  # the view that turns a bilinear or bicubic call into a launch of kind 2
_EXPECTED = {}  # filter -> the (oh, ow, 3) element bits of its views, shared by the layouts


@pytest.fixture(scope="module")
def sfiles(enc):  # noqa: F811
    """the sweep's image as a 3-channel file; its planes: the reference decoder's"""
    img = RS.image()
    f = _Files([bytes(p) for p in _encode_gpu(enc, [(img, 0)])], [(RS.SIZE, RS.SIZE)], [3])
    assert np.array_equal(f.planes[0][:3], img.transpose(2, 0, 1)) and (f.planes[0][3] == 255).all()
    return f


def _elements(planes3, mirror):
    return AM.view_elements(planes3, 3, "uint8", mirror, None, CONSTS[0], {}, {}, {}, {})


def _expected(sfiles, filter):
    if filter not in _EXPECTED:
        _EXPECTED[filter] = [_elements(p, m) for p, (_, _, m) in zip(RS.expected(sfiles.planes[0], filter), RS.views(filter))]
    return _EXPECTED[filter]


@pytest.mark.parametrize("filter", RS.FILTERS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_ratio_of_the_sweep(enc, sfiles, layout, filter):  # noqa: F811
    kinds = _kinds(layout)
    views = [(crop, full, None, filter, m, kinds[k % len(kinds)]) for k, (crop, full, m) in enumerate(RS.views(filter))]
    want = _expected(sfiles, filter)
    assert len(views) == len(want) == RS.PAIRS[filter]
    device = layout == "hwc"
    got, host, _, regs = _decode(enc, layout, sfiles.pngs, [(3, views)], "uint8", device, resample=True if filter not in VM.FILTERS else None)
    assert [(st, cf) for st, _, cf in got] == [(0, 3)]
    diff = _difference(layout, host, "uint8", regs, want)
    assert diff is None, (layout, filter, diff, [views[j][:2] for j, *_ in diff[4]])  # (the view: its crop's in_x, in_y and its out_x, out_y)
    if filter in VM.FILTERS:  # (the same views in a launch of kind 2)
        (x, y, w, h), full, m = NEAREST_VIEW
        more = views + [((x, y, w, h), full, None, "nearest", m, kinds[0])]
        got, mixed, _, regs = _decode(enc, layout, sfiles.pngs, [(3, more)], "uint8", device, resample=True)
        assert [(st, cf) for st, _, cf in got] == [(0, 3)]
        nearest = _elements(VM.view_planes(sfiles.planes[0][:3, y:y + h, x:x + w], full, None, "nearest"), m)
        diff = _difference(layout, mixed, "uint8", regs, want + [nearest])
        assert diff is None, (layout, filter, "with a NEAREST view", diff, [more[j][:2] for j, *_ in diff[4]])
        assert np.array_equal(mixed[:host.size], host)  # (the shared views' regions come first in both buffers)
