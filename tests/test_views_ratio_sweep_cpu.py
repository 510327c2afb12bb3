"""No-GPU companion of test_gpu_decode_views_ratios.py: it keeps the sweep of ratio_sweep.py honest.  The pair counts per filter; the
views' crops inside the image and at most four tiles each; and three MUTANTS of the model -- each a way a device compile of the
weight text could plausibly differ from the host's -- which must change bytes of at least one view of the real sweep, on the
sweep's own image: the box interval closed on the other side, first and count from the exact rational centre (what a fused
multiply-add would approximate), and NEAREST by the product form.  Needs no encoder: the image's planes are the image's own."""
from fractions import Fraction

import numpy as np
import pytest

import ratio_sweep as RS
import resample_model as SM
import resize_view_model as VM
from test_views_resample_cpu import PRODUCT_IS_WRONG

TILE_W, TILE_H = 64, 16  # resize.h: kResizeTileW, kResizeTileH


@pytest.fixture(scope="module")
def planes():
    p = np.ascontiguousarray(RS.image().transpose(2, 0, 1))
    p.setflags(write=False)
    return p


@pytest.fixture(scope="module")
def base(planes):
    """the model's views under the filters the mutants touch"""
    return {f: RS.expected(planes, f) for f in ("box", "nearest")}


def _clear():
    SM.axis_weights.cache_clear()
    SM._vm_axis_weights.cache_clear()


@pytest.fixture
def mutate(monkeypatch):
    """monkeypatch, with the models' weight caches emptied in front of the mutant and behind it"""
    _clear()
    yield monkeypatch
    monkeypatch.undo()
    _clear()


def _restated(in_size, out_size, filter, exact):
    """resize_view_model.axis_weights again; exact: first and count from center -/+ support + 0.5 in exact rationals"""
    kf = VM.KERNEL[filter]
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = VM.SUPPORT[filter] * fs
    ss = 1.0 / fs
    q_scale = Fraction(in_size, out_size)
    q_support = Fraction(VM.SUPPORT[filter]) * max(q_scale, 1)
    firsts, counts, weights = [], [], []
    for o in range(out_size):
        center = (o + 0.5) * scale
        if exact:
            q_center = (o + Fraction(1, 2)) * q_scale
            first = max(int(q_center - q_support + Fraction(1, 2)), 0)
            count = min(int(q_center + q_support + Fraction(1, 2)), in_size) - first
        else:
            first = max(int(center - support + 0.5), 0)
            count = min(int(center + support + 0.5), in_size) - first
        k = [kf(((t + first) - center + 0.5) * ss) for t in range(count)]
        ww = 0.0
        for v in k:
            ww += v
        if ww != 0.0:
            k = [v / ww for v in k]
        firsts.append(first)
        counts.append(count)
        weights.append([VM._fixed(v) for v in k])
    return firsts, counts, weights


def _changed(planes, base, filter, tables_differ):
    """(pairs whose axis tables the mutant changes, views of the sweep whose bytes it changes); the mutant is installed"""
    ps = RS.pairs(filter)
    moved = {p for p in ps if tables_differ(*p)}
    n = len(ps)
    only = {k for k in range(n) if ps[k] in moved or ps[n - 1 - k] in moved}
    got = RS.expected(planes, filter, only)
    return len(moved), sum(1 for k in only if not np.array_equal(got[k], base[filter][k]))


def test_the_pairs_and_the_views():
    """the counts per filter; every view: its crop inside the image, pair k in x and pair n - 1 - k in y, at most four tiles; the
    origins move"""
    for f in RS.FILTERS:
        ps, vs = RS.pairs(f), RS.views(f)
        assert len(ps) == len(vs) == RS.PAIRS[f], (f, len(ps))
        for k, ((x, y, w, h), (ow, oh), m) in enumerate(vs):
            assert (w, ow) == ps[k] and (h, oh) == ps[len(ps) - 1 - k] and m == bool(k & 1)
            assert 0 <= x and x + w <= RS.SIZE and 0 <= y and y + h <= RS.SIZE
            assert -(-ow // TILE_W) * -(-oh // TILE_H) <= 4
        assert len({(x, y) for (x, y, _, _), _, _ in vs}) > 100
    assert all(p in RS.pairs("nearest") for p in PRODUCT_IS_WRONG[:3])


def test_the_image_reaches_both_clips(planes):
    img = RS.image()
    assert img.shape == (RS.SIZE, RS.SIZE, 3) and set(np.unique(img[::2])) == {0, 255} and set(np.unique(img[:, ::2])) == {0, 255} and len(np.unique(img[1::2, 1::2])) == 256
    sums = VM.one_pass_sums(planes[0, :, :96], 64, "lanczos") >> VM.PRECISION_BITS
    assert sums.min() < 0 and sums.max() > 255


def test_the_restatement_is_the_model():
    """_restated(exact=False) is resize_view_model.axis_weights on every pair of the sweep: the exact mutant differs from the model in
    first and count alone"""
    for f in ("box", "hamming", "lanczos", "bilinear", "bicubic"):
        assert all(_restated(i, o, f, False) == SM.axis_weights(i, o, f) for i, o in RS.pairs(f)), f


def test_mutant_box_closed_on_the_other_side(planes, base, mutate):
    want = {p: SM.axis_weights(*p, "box") for p in RS.pairs("box")}
    _clear()
    mutate.setitem(VM.KERNEL, "box", lambda a: 1.0 if -0.5 <= a < 0.5 else 0.0)
    pairs, views = _changed(planes, base, "box", lambda i, o: SM.axis_weights(i, o, "box") != want[(i, o)])
    print("box closed on the other side: pairs with other weights", pairs, "views with other bytes", views)
    assert pairs >= 1 and views >= 1


def test_mutant_first_and_count_from_the_exact_centre(planes, base, mutate):
    want = {p: SM.axis_weights(*p, "box") for p in RS.pairs("box")}
    _clear()
    mutate.setattr(VM, "axis_weights", lambda i, o, f="bilinear": _restated(i, o, f, True))
    pairs, views = _changed(planes, base, "box", lambda i, o: _restated(i, o, "box", True)[:2] != want[(i, o)][:2])
    print("exact centre under box: pairs with other taps", pairs, "views with other bytes", views)
    assert pairs >= 1 and views >= 1


def test_mutant_nearest_by_the_product_form(planes, base, mutate):
    running_sum = SM.nearest_indices
    mutate.setattr(SM, "nearest_indices", SM.product_indices)
    pairs, views = _changed(planes, base, "nearest", lambda i, o: SM.product_indices(i, o) != running_sum(i, o))
    print("nearest by the product form: pairs with another index table", pairs, "views with other bytes", views)
    assert pairs >= 1 and views >= 1
    assert all(SM.product_indices(*p) != running_sum(*p) for p in PRODUCT_IS_WRONG[:3])
