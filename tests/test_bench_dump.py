"""bench.py --dump-outputs without a GPU: dump_outputs() on stand-in output buffers of the sizes real batches have.  Whatever the batch
and file sizes, the files written stay within the budget (64 MB is the cap), every index lies in its file, the values are that file's
bytes there, small files are written whole, and the same outputs give the same dump."""
import os
import sys
import zlib

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _dump(tmp_path, name, batch, size):
    import bench
    data = torch.from_numpy(np.random.default_rng(size).integers(0, 256, size + 64, dtype=np.uint8))
    sizes = [max(1, size - i % 7) for i in range(batch)]
    res = [(s, i & 1, 0) for i, s in enumerate(sizes)]
    d = str(tmp_path / name)
    bench.dump_outputs(d, [data] * batch, res, 0, 1)  # (one buffer stands in for all of them: the sizes differ)
    return d, data.numpy(), sizes


@pytest.mark.parametrize("batch,size", [(1024, 372_000),   # --workload 512 --batch 1024: sampled, a small share each
                                        (8, 60_000_000),   # 8K frames: sampled, a large share each
                                        (8, 1000),         # written whole
                                        (4000, 3000)])     # files larger than their share and smaller than 4096 bytes
def test_dump_fits_the_budget_and_holds_the_files_bytes(tmp_path, batch, size):
    import bench
    d, data, sizes = _dump(tmp_path, "a", batch, size)
    names = os.listdir(d)
    assert len(names) == 2 * batch + 1
    total = sum(os.path.getsize(os.path.join(d, n)) for n in names)
    assert total <= bench.DUMP_BUDGET <= 64_000_000, total
    info = np.load(os.path.join(d, "png_info.npy"))
    per_file = bench.dump_per_file(batch)
    for i in sorted({0, 1, batch // 2, batch - 1}):
        f = data[: sizes[i]]
        assert tuple(info[i]) == (sizes[i], i & 1, 0, zlib.crc32(f.tobytes()))
        idx = np.load(os.path.join(d, f"png_{i}_index.npy"))
        val = np.load(os.path.join(d, f"png_{i}.npy"))
        assert idx.dtype == np.float64 and val.dtype == np.float32 and idx.shape == val.shape
        ix = idx.astype(np.int64)
        assert (ix == idx).all() and (np.diff(ix) > 0).all() and ix[0] >= 0 and ix[-1] < sizes[i]
        assert (val == f[ix]).all()
        if sizes[i] <= per_file:
            assert (ix == np.arange(sizes[i])).all()
        else:
            e = min(4096, per_file // 4)
            assert e > 0 and len(ix) <= per_file
            assert (ix[:e] == np.arange(e)).all() and (ix[-e:] == np.arange(sizes[i] - e, sizes[i])).all()


def test_the_same_outputs_give_the_same_dump(tmp_path):
    a, _, _ = _dump(tmp_path, "a", 8, 2_000_000)
    b, _, _ = _dump(tmp_path, "b", 8, 2_000_000)
    for n in sorted(os.listdir(a)):
        assert np.array_equal(np.load(os.path.join(a, n)), np.load(os.path.join(b, n))), n
