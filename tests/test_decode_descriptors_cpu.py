"""CPU tests of the rules that the eight decode-descriptor makers (Encoder.make_decode_batch_ex, _planar, _float, _crop, _resize,
_resize_view, _views, _views_hwc) and the calls that run their descriptors share: per-file lists of the wrong length, host files
kept alive by the descriptor, another call's descriptor refused before the library is touched, and pixels_cap as the destination
view's own span.  The makers read strides and addresses only, so CPU tensors stand in for the device's.  No GPU."""
import ctypes
import gc

import pytest
import torch

import fpng_amd
from fpng_amd import Encoder

W, H = 4, 2  # every destination's size, and every crop's
CROP = (0, 0, W, H)
N = 3


class _OnDevice(torch.Tensor):
    is_cuda = True  # a CPU tensor that says it is a CUDA one: make_decode_batch_ex asks its destinations


def _canvas(kind, dtype):
    """a canvas larger than a destination, and the strided crop of it that is the destination of `kind`"""
    if kind == "ex":
        big = torch.zeros(H + 3, W + 5, 4, dtype=dtype).as_subclass(_OnDevice)
        return big, big[1:1 + H, 2:2 + W]
    if kind == "views_hwc":
        big = torch.zeros(H + 3, W + 5, 4, dtype=dtype)
        return big, big[1:1 + H, 2:2 + W, :3]
    big = torch.zeros(4, H + 3, W + 5, dtype=dtype)
    return big, big[:3, 1:1 + H, 2:2 + W]


def _dtype(kind):
    return torch.float16 if kind == "float" else torch.uint8


def _make(kind, files, outs, **kw):
    n = len(files)
    if kind in ("ex", "planar", "float"):
        return getattr(Encoder, "make_decode_batch_" + kind)(files, outs, **kw)
    if kind == "crop":
        return Encoder.make_decode_batch_crop(files, [CROP] * n, outs, **kw)
    if kind == "resize":
        return Encoder.make_decode_batch_resize(files, [(1, 1, 9, 7)] * n, outs, **kw)
    if kind == "resize_view":
        return Encoder.make_decode_batch_resize_view(files, [(1, 1, 9, 7)] * n, outs, (W, H), **kw)
    return getattr(Encoder, "make_decode_batch_" + kind)(files, [[(1, 1, 9, 7)]] * n, [[t] for t in outs], (W, H), **kw)


KINDS = ("ex", "planar", "float", "crop", "resize", "resize_view", "views", "views_hwc")
CLASSES = {"ex": fpng_amd.DecodeBatchEx, "planar": fpng_amd.DecodeBatchPlanar, "float": fpng_amd.DecodeBatchFloat, "crop": fpng_amd.DecodeBatchCrop,
           "resize": fpng_amd.DecodeBatchResize, "resize_view": fpng_amd.DecodeBatchResizeView, "views": fpng_amd.DecodeBatchMultiView,
           "views_hwc": fpng_amd.DecodeBatchMultiViewHwc}
FILES = [b"\x89PNG-one", b"", b"three"]


def _outs(kind, n=N, dtype=None):
    return [_canvas(kind, dtype or _dtype(kind))[1] for _ in range(n)]


@pytest.mark.parametrize("kind", KINDS)
def test_every_maker_makes_its_own_class(kind):
    d = _make(kind, FILES, _outs(kind), order=["rgb", "bgr", "rgb"], bottom_up=[False, True, False])
    assert type(d) is CLASSES[kind] and type(d).maker == "make_decode_batch_" + kind and not d.device_data
    assert len(d.arr) == len(d.res) == N and list(d.statuses()) == [0] * N
    assert CLASSES[kind].call(True) == "decode_device_" + kind and CLASSES[kind].call(False) == "decode_batch_" + kind


# (the calls without a resize take no mirror flags)
PER_FILE = [(kind, arg) for kind in KINDS for arg in ("order", "bottom_up", "mirror") if arg != "mirror" or kind not in ("ex", "planar", "float", "crop")]


@pytest.mark.parametrize("length", [N - 1, N + 1, 0])
@pytest.mark.parametrize("kind,arg", PER_FILE)
def test_a_per_file_list_of_the_wrong_length_is_refused(kind, arg, length):
    """order, bottom_up and mirror: one value, or one per file -- a list that is shorter or longer than the files is a ValueError in
    every maker, none truncates it"""
    one = {"order": "rgb", "bottom_up": True, "mirror": True}[arg]
    assert _make(kind, FILES, _outs(kind), **{arg: [one] * N}) is not None
    with pytest.raises(ValueError, match="make_decode_batch_" + kind):
        _make(kind, FILES, _outs(kind), **{arg: [one] * length})


@pytest.mark.parametrize("kind", KINDS)
def test_destinations_as_many_as_files(kind):
    for n in (N - 1, N + 1):
        with pytest.raises(ValueError, match="make_decode_batch_" + kind):
            if kind.startswith("views"):
                getattr(Encoder, "make_decode_batch_" + kind)(FILES, [[CROP]] * N, [[t] for t in _outs(kind, n)], (W, H))
            else:
                _make(kind, FILES, _outs(kind, n))


@pytest.mark.parametrize("kind", KINDS)
def test_host_files_are_kept_alive_by_the_descriptor(kind):
    """the records point into copies the descriptor keeps: the caller's buffers may go"""
    texts = [b"\x89PNG-one", b"", b"three, which is longer"]

    def build():
        files = [bytearray(t) for t in texts]  # (mutable: the maker has to copy them)
        d = _make(kind, files, _outs(kind))
        for f in files:
            f[:] = b"\0" * len(f)
        return d

    d = build()
    gc.collect()
    assert not d.device_data and len(d._keep) == N
    for i, text in enumerate(texts):
        assert d.arr[i].size == len(text)
        if text:
            assert d.arr[i].data == d._keep[i].ctypes.data and ctypes.string_at(d.arr[i].data, d.arr[i].size) == text
        else:
            assert d.arr[i].data is None


def _span(t):
    """bytes from a view's first element to behind its last, from its shape and strides alone"""
    return (sum((n - 1) * s for n, s in zip(t.shape, t.stride())) + 1) * t.element_size()


# (the _ex and _planar calls write bytes, the _float call floats, the others either)
DEST_DTYPES = [(kind, dtype) for kind in KINDS for dtype in (torch.uint8, torch.float16, torch.float32)
               if (dtype is torch.uint8) != (kind == "float") and (dtype is torch.uint8 or kind not in ("ex", "planar"))]


@pytest.mark.parametrize("kind,dtype", DEST_DTYPES)
def test_pixels_cap_is_the_views_own_span(kind, dtype):
    """a strided crop of a larger canvas, bottom-up and with the planes / channels reversed: the room check covers the view, from its
    lowest address, and nothing of the canvas around it"""
    big, t = _canvas(kind, dtype)
    assert not t.is_contiguous() and _span(t) < big.numel() * big.element_size()
    for order, up in (("rgb", False), ("bgr", True)):
        d = _make(kind, FILES[:1], [t], order=order, bottom_up=up)
        rec = d.dests[0] if kind.startswith("views") else d.arr[0]
        assert rec.pixels_cap == _span(t), (order, up)
        # the lowest address the record's pitches reach is the view's first element
        c, h = (t.shape[0], t.shape[1]) if kind not in ("ex", "views_hwc") else (t.shape[2], t.shape[0])
        low = rec.d_pixels + min(0, (h - 1) * rec.row_pitch)
        if kind not in ("ex", "views_hwc"):
            low += min(0, (c - 1) * rec.plane_pitch)
        assert low == t.data_ptr() and (rec.row_pitch < 0) == up, (order, up)


@pytest.fixture(scope="module")
def descriptors():
    made = {kind: _make(kind, FILES, _outs(kind)) for kind in KINDS}
    made["legacy"] = fpng_amd.api.DecodeBatch([], [], None, None, 3)  # (what make_decode_batch() returns)
    return made


@pytest.mark.parametrize("device", [True, False])
@pytest.mark.parametrize("kind", KINDS)
def test_another_calls_descriptor_is_refused(descriptors, kind, device):
    """every call takes its own maker's descriptors only: any other is a ValueError that names that maker, raised before the call
    touches the library or the device (the encoder here has neither)"""
    e = Encoder.__new__(Encoder)
    fn = getattr(Encoder, ("decode_device_" if device else "decode_batch_") + kind)
    for other, d in descriptors.items():
        if other == kind:
            continue
        with pytest.raises(ValueError, match=r"make_decode_batch_" + kind + r"\(\)") as err:
            fn(e, d)
        assert fn.__name__ in str(err.value), other
    # its own descriptor passes that check: of host files, the device call says so; the host call reaches the CPU destinations
    # (the _ex maker has refused those itself)
    if device or kind != "ex":
        with pytest.raises(ValueError, match="host memory" if device else "CUDA"):
            fn(e, descriptors[kind])
