"""CPU tests of the encode descriptors: the image records of the four source kinds (plain HWC `image`, strided / BGR(A) `ex`,
`planar` uint8, planar `float`) are built in one place, so the makers with outputs (Encoder.make_batch, _ex, _planar, _float),
make_batch_packed and the renditions calls describe the same tensors with the same records -- which are what the tensors' own
addresses and strides say.  Then the rules the makers share (lists of the wrong length, another call's descriptor) and what every
submit method ends in (the ticket, the buffers kept alive for the eight submissions that can be in flight), against a stub of
the library.  The makers read strides and addresses only, so CPU tensors stand in for the device's.  No GPU."""
import ctypes as C

import pytest
import torch

import fpng_amd
from fpng_amd import Encoder, _lib
from fpng_amd.api import _source_records
from fpng_amd.api import denormalize_constants

W, H = 4, 2  # every image's size
CHANS = (3, 4, 3)
N = len(CHANS)
KINDS = ("image", "ex", "planar", "float")
MAKERS = {"image": Encoder.make_batch, "ex": Encoder.make_batch_ex, "planar": Encoder.make_batch_planar, "float": Encoder.make_batch_float}
SUBMITS = {"image": Encoder.submit, "ex": Encoder.submit_ex, "planar": Encoder.submit_planar, "float": Encoder.submit_float}
RECORDS = {"image": _lib.Image, "ex": _lib.ImageEx, "planar": _lib.ImagePlanar, "float": _lib.ImagePlanar}
FLOATS = {torch.float32: _lib.F32, torch.float16: _lib.F16, torch.bfloat16: _lib.BF16}
CASES = [(kind, dtype) for kind in KINDS for dtype in (FLOATS if kind == "float" else (torch.uint8,))]


class _OnDevice(torch.Tensor):
    is_cuda = True  # a CPU tensor that says it is a CUDA one: make_batch and make_batch_ex ask their tensors


def _images(kind, dtype=torch.uint8):
    """a 4 x 2 image per entry of CHANS: tight rows for the plain kind (it takes nothing else), for the others a strided crop of a
    larger canvas -- of 4-byte pixels for `ex`, so that the 3-channel ones are RGBX"""
    if kind == "image":
        return [torch.zeros(H, W, c, dtype=dtype).as_subclass(_OnDevice) for c in CHANS]
    if kind == "ex":
        return [torch.zeros(H + 3, W + 5, 4, dtype=dtype).as_subclass(_OnDevice)[1:1 + H, 2:2 + W, :c] for c in CHANS]
    return [torch.zeros(4, H + 3, W + 5, dtype=dtype)[:c, 1:1 + H, 2:2 + W] for c in CHANS]


def _outs(n=N):
    return [torch.zeros(100 + 16 * i, dtype=torch.uint8).as_subclass(_OnDevice) for i in range(n)]


def _layouts(kind):
    """the layout arguments of a kind's calls, as one value and as a list per image, and what they mean for each image"""
    if kind == "image":
        return [({}, ["rgb"] * N, [False] * N)]
    rev = ["bgr" if kind == "ex" or c == 3 else "abgr" for c in CHANS]  # (planes: one pitch says R..A or A..R only)
    orders, ups = ["rgb", rev[1], rev[2]], [False, True, True]
    return [({}, ["rgb"] * N, [False] * N), (dict(order="rgb", bottom_up=True), ["rgb"] * N, [True] * N),
            (dict(order=orders, bottom_up=ups), orders, ups)]


def _expected(kind, t, order, up):
    """a record's fields from the view's address, shape and strides alone"""
    if kind == "image":
        return dict(d_pixels=t.data_ptr(), w=t.shape[1], h=t.shape[0], num_chans=t.shape[2])
    e = t.element_size()
    if kind == "ex":
        h, w, c = t.shape
        assert t.data_ptr() % 4 == 0 and t.stride(1) == 4 and not t.is_contiguous()
        name = order.upper() + ("A" if c == 4 else "X")  # (the byte a 3-channel view leaves out lies behind its channels)
        return dict(d_pixels=t.data_ptr() + ((h - 1) * t.stride(0) if up else 0), row_pitch=-t.stride(0) if up else t.stride(0), w=w, h=h,
                    format=fpng_amd.SRC_FORMATS[name][0])
    c, h, w = t.shape
    assert not t.is_contiguous()
    plane, row = t.stride(0) * e, t.stride(1) * e
    rev = order[0] != "r"
    return dict(d_pixels=t.data_ptr() + ((c - 1) * plane if rev else 0) + ((h - 1) * row if up else 0), row_pitch=-row if up else row,
                plane_pitch=-plane if rev else plane, w=w, h=h, num_chans=c, reserved=0)


def _fields(rec, but=()):
    return {name: getattr(rec, name) for name, _ in rec._fields_ if name not in but}


@pytest.mark.parametrize("kind,dtype", CASES)
def test_every_path_builds_the_same_records(built_lib, kind, dtype):
    images, outs = _images(kind, dtype), _outs()
    constants = dict(mean=(0.5, 0.25, 0.125), std=(0.5, 0.25, 2.0)) if kind == "float" else {}
    for layout, orders, ups in _layouts(kind):
        layout = dict(layout, **constants)
        made = MAKERS[kind](images, outs, **layout)
        packed = Encoder.make_batch_packed(images, kind, **layout)
        plain = _source_records("submit_renditions", images, kind, **layout)  # (as submit_renditions and renditions_plan call it)
        assert made[:2] == (images, outs) and len(made) == (4 if kind == "float" else 3)
        assert packed[:3] == ("packed", kind, images) and len(packed) == (6 if kind == "float" else 5)
        for arr in (made[2], packed[4], plain[0]):
            assert isinstance(arr, C.Array) and arr._type_ is RECORDS[kind] and len(arr) == N
        for i, (t, out, order, up) in enumerate(zip(images, outs, orders, ups)):
            want = _expected(kind, t, order, up)
            assert _fields(made[2][i], ("d_out", "out_cap")) == want, (layout, i)
            assert (made[2][i].d_out, made[2][i].out_cap) == (out.data_ptr(), out.numel())
            for arr in (packed[4], plain[0]):
                assert _fields(arr[i]) == dict(want, d_out=None, out_cap=0), (layout, i)
        if kind == "float":
            sc, bi = denormalize_constants(constants["mean"], constants["std"])
            for fmt in (made[3], packed[5], plain[1]):
                assert (fmt.dtype, fmt.reserved) == (FLOATS[dtype], 0)
                assert list(fmt.scale) == [float(v) for v in sc] and list(fmt.bias) == [float(v) for v in bi]
        else:
            assert plain[1] is None
        # the library takes these records for a renditions call: each image at its own size
        total, offs = fpng_amd.renditions_plan(images, [fpng_amd.rendition(i, (W, H)) for i in range(N)], kind, packed=True, **layout)
        assert len(offs) == N and total > 0


def test_make_batch_refuses_with_a_value_error():
    """what were bare asserts: every refusal names the call"""
    good, outs = _images("image"), _outs()
    assert Encoder.make_batch(good, outs)[2][1].num_chans == 4
    for bad in (torch.zeros(H, W, 3, dtype=torch.uint8),                                   # not on the device
                torch.zeros(H, W, 3, dtype=torch.float32).as_subclass(_OnDevice),         # not bytes
                torch.zeros(H, 2 * W, 3, dtype=torch.uint8).as_subclass(_OnDevice)[:, ::2],  # not contiguous
                torch.zeros(H * W * 3, dtype=torch.uint8).as_subclass(_OnDevice)):         # not (h, w, c)
        with pytest.raises(ValueError, match="make_batch"):
            Encoder.make_batch([good[0], bad], outs[:2])
    ex = _images("ex")
    with pytest.raises(ValueError, match="make_batch_ex.*CUDA"):
        Encoder.make_batch_ex([ex[0].as_subclass(torch.Tensor)], outs[:1])
    with pytest.raises(ValueError, match="make_batch_ex.*CUDA"):
        Encoder.make_batch_ex(ex[:1], [torch.zeros(100, dtype=torch.uint8)])


@pytest.mark.parametrize("length", [N - 1, N + 1, 0])
@pytest.mark.parametrize("kind", KINDS)
def test_a_list_of_the_wrong_length_is_refused(kind, length):
    """outs, order and bottom_up: a list that is shorter or longer than the images is a ValueError in every maker, none truncates it"""
    dtype = torch.float16 if kind == "float" else torch.uint8
    images = _images(kind, dtype)
    name = MAKERS[kind].__name__
    with pytest.raises(ValueError, match=name):
        MAKERS[kind](images, _outs(length))
    if kind == "image":
        return
    for arg, one in (("order", "rgb"), ("bottom_up", True)):
        assert len(MAKERS[kind](images, _outs(), **{arg: [one] * N})[2]) == N
        with pytest.raises(ValueError, match=name):
            MAKERS[kind](images, _outs(), **{arg: [one] * length})
        with pytest.raises(ValueError, match="make_batch_packed"):
            Encoder.make_batch_packed(images, kind, **{arg: [one] * length})
        with pytest.raises(ValueError, match="renditions_plan"):
            fpng_amd.renditions_plan(images, [fpng_amd.rendition(0, (W, H))], kind, **{arg: [one] * length})


@pytest.fixture(scope="module")
def descriptors():
    made = {kind: MAKERS[kind](_images(kind, torch.float16 if kind == "float" else torch.uint8), _outs()) for kind in KINDS}
    made["packed"] = Encoder.make_batch_packed(_images("image"))
    return made


@pytest.mark.parametrize("kind", KINDS + ("packed",))
def test_another_calls_descriptor_is_refused(descriptors, kind):
    """every submit method takes its own maker's descriptors only: any other is a ValueError raised before the call touches the
    library or the device (the encoder here has neither)"""
    e = Encoder.__new__(Encoder)
    arena = torch.zeros(4096, dtype=torch.uint8).as_subclass(_OnDevice)
    for other, d in descriptors.items():
        if other == kind:
            continue
        with pytest.raises(ValueError, match="make_batch"):
            if kind == "packed":
                Encoder.submit_packed(e, d, arena)
            else:
                SUBMITS[kind](e, d)
    # (the images of a call without outs are a descriptor, never tensors)
    if kind != "packed":
        with pytest.raises(ValueError, match="make_batch"):
            SUBMITS[kind](e, _images(kind, torch.float16 if kind == "float" else torch.uint8))


class _StubLib:
    """a library whose submit functions hand out rising tickets and whose waits succeed: `calls` lists the functions called"""

    def __init__(self):
        self.ticket, self.calls = 0, []

    def __getattr__(self, name):
        if not name.startswith(("fpng_amd_encode_submit", "fpng_amd_encode_wait", "fpng_amd_encode_finish")):
            raise AttributeError(name)

        def fn(*args):
            self.calls.append(name)
            if "submit" in name:
                self.ticket += 1
                args[-1]._obj.value = self.ticket  # (the ticket is every submit function's last argument, by reference)
            return 0
        return fn


def _stub_encoder():
    e = Encoder.__new__(Encoder)
    e.lib, e.h, e._keep, e._follow_torch = _StubLib(), None, {}, False
    return e


def _on_device(batch):
    return tuple([t.as_subclass(_OnDevice) for t in part] if isinstance(part, list) else part for part in batch)


def test_the_runner_keeps_the_buffers_of_eight_submissions():
    e = _stub_encoder()
    batches = {kind: _on_device(MAKERS[kind](_images(kind, torch.float16 if kind == "float" else torch.uint8), _outs())) for kind in KINDS}
    arena = torch.zeros(4096, dtype=torch.uint8).as_subclass(_OnDevice)
    table = torch.zeros(2 * (N + 1), dtype=torch.int64).as_subclass(_OnDevice)
    packed = Encoder.make_batch_packed(_images("image"))
    for round_ in range(5):
        for kind in KINDS:
            assert SUBMITS[kind](e, batches[kind]) == N  # a prebuilt descriptor: the one C call
            assert e.last_ticket == e.lib.ticket and e._keep[e.last_ticket] is batches[kind]
            assert sorted(e._keep) == list(range(max(1, e.last_ticket - 7), e.last_ticket + 1))
        assert e.submit_packed(packed, arena, table=table) == N
        kept = e._keep[e.last_ticket]
        assert kept[0] is packed and kept[1] is arena and kept[2] is table  # the arena and the table live as long as the sources
        assert len(e._keep) <= 8
        rends = [fpng_amd.rendition(i, (W, H)) for i in range(N)]
        assert e.submit_renditions(batches["image"][0], rends, arena=arena, table=table) == N
        kept = e._keep[e.last_ticket]
        assert all(a is b for a, b in zip(kept[0], batches["image"][0])) and kept[2] is arena and kept[3] is table and len(e._keep) <= 8
    assert e.lib.calls == ["fpng_amd_encode_submit", "fpng_amd_encode_submit_ex", "fpng_amd_encode_submit_planar", "fpng_amd_encode_submit_planar_float",
                           "fpng_amd_encode_submit_packed", "fpng_amd_encode_submit_renditions"] * 5
    assert e.last_ticket == 30 and sorted(e._keep) == list(range(23, 31))
    # a wait drops its ticket's buffers, finish() everyone's
    e.wait(30, N)
    e.wait_packed(29, N)
    assert sorted(e._keep) == list(range(23, 29))
    e.wait(5, N)  # (long gone: nothing to drop)
    assert sorted(e._keep) == list(range(23, 29))
    e.finish(N)
    assert e._keep == {}
