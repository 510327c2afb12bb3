"""The decoder's synchronisation on the GPU, branch by branch (-m gpu; dec_sync_kernel, dec_chain_kernel, dec_offsets_kernel and
dec_subscan_kernel of fpng_amd/csrc/decode.hip): the files of tests/sync_cases.py -- streams that end on, in front of and across
subsequence and workgroup borders, blocks with 0, 1 .. 3, 4, 64, 65 and more threads to correct, blocks left to round 1's phase
maps, batches of 1, 63, 64 and 65 files with stored files among them, windows with the most walks a file can have.
tests/test_sync_cases_cpu.py holds every file to the property it is named for; here the kernels must decode each one to the judge's
pixels with status 0 -- FPNG_AMD_DECODE_UNDECIDED is never accepted: the files are valid, the CPU tier must not hide a miss --
from host memory and from device memory at every offset (mod 4) of the file, alone and as a batch, to 3 and to 4 channels."""
import struct

import numpy as np
import pytest

import sync_cases as S
from test_gpu_decode import _device_files, enc, judge  # noqa: F401  (enc: the module's fixture)

pytestmark = pytest.mark.gpu
PLACES = ("host", 0, 1, 2, 3)  # host memory; device memory, the file's first byte at this offset from a dword boundary

_expected = {}


def _want(png, desired):
    """the judge's pixels of a file (judged once)"""
    key = (png, desired)
    if key not in _expected:
        st, px, w, h, c = judge(png, desired)
        assert st == 0
        _expected[key] = (np.asarray(px)[: w * h * desired].copy(), w, h, c)
    return _expected[key]


def _decode(enc, pngs, desired, place):
    if place == "host":
        return enc.decode_batch(pngs, desired)
    dev = [_device_files([p], shift=place)[0] for p in pngs]  # (every file at the same offset)
    assert all(d.data_ptr() % 4 == place for d in dev)
    return enc.decode_device(dev, desired, [struct.unpack(">II", p[16:24]) for p in pngs])


def _hold(got, pngs, desired, what):
    assert len(got) == len(pngs)
    for k, ((st, px, cf), png) in enumerate(zip(got, pngs)):
        exp, w, h, c = _want(png, desired)
        assert st == 0, (what, k, st)
        assert cf == c and tuple(px.shape) == (h, w, desired), (what, k)
        assert np.array_equal(px.cpu().numpy().reshape(-1), exp), (what, k)


def _group(enc, cases, desired):
    names, pngs = [c.name for c in cases], [c.png for c in cases]
    for place in PLACES:
        _hold(_decode(enc, pngs, desired, place), pngs, desired, ("batch", place, names))
        for name, png in zip(names, pngs):
            _hold(_decode(enc, [png], desired, place), [png], desired, (name, place))


@pytest.fixture(scope="module")
def cases():
    return S.all_cases()


@pytest.mark.parametrize("desired", [3, 4])
def test_stream_ends_at_subsequence_and_workgroup_borders(enc, cases, desired):
    """Group A: the end-of-block code begins on, ends on and straddles a border inside a workgroup's block and the border between two
    blocks (then block 1 is one subsequence with the code's tail, or with padding bits alone); 1, 2, 511, 512, 513, 1024 and 1025
    subsequences; the first token at bit 0, 1, 31 of a dword and in between."""
    _group(enc, cases["A"], desired)


@pytest.mark.parametrize("desired", [3, 4])
def test_round_0_corrects_none_few_and_many_threads(enc, cases, desired):
    """Group B: blocks whose first step has 0, 1, 2, 3 (decoded again in place), 4, 5 .. 63, 64, 65 and more than 128 threads to
    correct (gathered into wave 0, in one pass and in several), second and third steps, blocks left to round 1 and its phase maps,
    settled blocks that a border round opens, gathered threads in every wave and in a short last block."""
    _group(enc, cases["B"], desired)


@pytest.mark.parametrize("desired", [3, 4])
def test_windows_with_the_most_walks(enc, cases, desired):
    """Group D: rows of 12-bit literals alone -- 42 bytes per subsequence, 26 (20) walks in a window of 256 four-byte (three-byte)
    pixels, the most a file the GPU path takes can have."""
    _group(enc, cases["D"], desired)


def test_round_0_cases_into_planes(enc, cases):
    """Group B through decode_device_planar (the synchronisation is shared by every entry point: one other is enough)."""
    import torch
    pngs = [c.png for c in cases["B"]]
    dims = [struct.unpack(">II", p[16:24]) for p in pngs]
    views = [torch.zeros((4, h, w), dtype=torch.uint8, device="cuda") for w, h in dims]
    got = enc.decode_device_planar(_device_files(pngs, shift=1), views)
    for k, ((st, v, cf), png) in enumerate(zip(got, pngs)):
        exp, w, h, c = _want(png, 4)
        assert st == 0 and cf == c, (cases["B"][k].name, st)
        assert np.array_equal(v.permute(1, 2, 0).contiguous().cpu().numpy().reshape(-1), exp), cases["B"][k].name


@pytest.mark.parametrize("desired", [3, 4])
def test_batches_around_64_files_with_stored_files_among_them(enc, cases, desired):
    """Group C: 1, 63, 64 and 65 compressed files (most with 1 to 3 subsequences, two with two blocks), stored files first, in the
    middle and last -- they own no subsequences and share their successor's sub_base --, 64 and 65 without any, and 64 files with
    stored ones among them (job_of_sub_wave's ballot).  Every batch against the judge and against its files decoded one per call."""
    import torch
    single = {}
    for batch in cases["C"]:
        for f in batch.files:
            if f not in single:
                (st, px, cf), = enc.decode_batch([f], desired)
                _hold([(st, px, cf)], [f], desired, (batch.name, "alone"))
                single[f] = px
        for place in ("host", 1):
            if place == "host":
                got = enc.decode_batch(batch.files, desired)
            else:  # (offsets dealt round-robin)
                got = enc.decode_device(_device_files(batch.files, shift=1), desired, [struct.unpack(">II", p[16:24]) for p in batch.files])
            _hold(got, batch.files, desired, (batch.name, place))
            for k, ((st, px, cf), f) in enumerate(zip(got, batch.files)):
                assert torch.equal(px, single[f]), (batch.name, place, k)
