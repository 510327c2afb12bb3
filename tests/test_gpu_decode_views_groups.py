"""GPU test of the views calls' record indexing across GROUPS of files when a file in the middle gets no job: three large stored
host files -- several groups -- whose middle file's crop leaves the image, the other two with a direct view, a blur view and a tone
view each.  Every view must be byte-equal to the same view decoded alone in a one-file call of the same entry point, and the middle
file's destinations stay untouched.  The second test does the same under RESAMPLE records -- NEAREST index tables next to the file
without a job, groups whose launches differ in kind and in the alpha instantiation -- and holds every view against the model too."""
import pytest

from test_gpu_decode_layouts import SENTINEL
from test_gpu_decode_resize import CROP_OUTSIDE, enc  # noqa: F401  (enc: a fixture)
from test_gpu_decode_views import big_files  # noqa: F401  (a fixture)
from test_gpu_decode_views_alpha import _Model
from test_gpu_decode_views_color import _difference
from test_gpu_decode_views_resample_alpha import NONE, PRE, _decode, _kinds, _sources
from test_gpu_decode_views_tone import EQUAL

pytestmark = pytest.mark.gpu

# per file: (crop, full size, window) of its views -- windows of at most 64 x 16 -- as direct, blur and tone view
VIEWS = [[((1000, 1000, 24, 24), (12, 12), None), ((3, 5, 130, 64), (65, 32), (1, 2, 64, 16)), ((500, 700, 64, 48), (32, 24), (3, 5, 25, 13))],
         [((1000, 1000, 25, 24), (12, 12), None), ((0, 0, 40, 30), (20, 15), None), ((10, 10, 16, 16), (8, 8), None)],  # (1000 + 25 > 1024: outside)
         [((0, 0, 9, 9), (27, 27), (20, 20, 7, 7)), ((1015, 0, 9, 1024), (3, 64), (0, 8, 3, 16)), ((512, 512, 96, 32), (48, 16), None)]]


def _size(full, window):
    return (window[2], window[3]) if window is not None else full


@pytest.mark.parametrize("hwc", [False, True])
def test_tone_views_in_several_groups_around_a_file_without_a_job(enc, big_files, hwc):  # noqa: F811
    import fpng_amd
    import torch
    records = [[fpng_amd.view_post(), fpng_amd.view_post(blur=(5, 1.3)), fpng_amd.view_post(solarize=100)]] * 3
    tones = [[fpng_amd.view_tone(), fpng_amd.view_tone(), fpng_amd.view_tone(equalize=(i == 0), autocontrast=(i != 0))] for i in range(3)]
    call = enc.decode_batch_views_hwc if hwc else enc.decode_batch_views

    def decode(idx):
        outs = [[torch.full((h, w, 3) if hwc else (3, h, w), SENTINEL, dtype=torch.uint8, device="cuda") for w, h in (_size(f, win) for _, f, win in VIEWS[i])] for i in idx]
        got = call([big_files.pngs[i] for i in idx], [[v[0] for v in VIEWS[i]] for i in idx], outs, [[v[1] for v in VIEWS[i]] for i in idx],
                   [[v[2] for v in VIEWS[i]] for i in idx], filter=[["bilinear", "bicubic", "bilinear"]] * len(idx), mirror=[[False, True, False]] * len(idx),
                   post=[records[i] for i in idx], tone=[tones[i] for i in idx])
        torch.cuda.synchronize()
        return [st for st, _, _ in got], [[t.cpu() for t in ts] for ts in outs]

    statuses, together = decode([0, 1, 2])
    assert statuses == [0, CROP_OUTSIDE, 0]
    for i in (0, 2):
        (st,), (alone,) = decode([i])
        assert st == 0
        for k, (a, b) in enumerate(zip(together[i], alone)):
            assert not bool((b == SENTINEL).all()) and torch.equal(a, b), (hwc, i, k)
    assert all(bool((t == SENTINEL).all()) for t in together[1])


# per file: (crop, full size, window, filter) of its views.  File 0: a NEAREST direct view, a Lanczos view in front of a blur, a box
# view in front of a tone op; file 1: its first crop leaves the image, a NEAREST view among its views; file 2: bilinear and bicubic
# views whose records carry no filter, so its group launches kinds 0 / 1 where file 0's launches kind 2
RESAMPLE_VIEWS = [[((1000, 1000, 24, 24), (12, 12), None, "nearest"), ((3, 5, 130, 64), (65, 32), (1, 2, 64, 16), "lanczos"), ((500, 700, 64, 48), (32, 24), (3, 5, 25, 13), "box")],
                  [((1000, 1000, 25, 24), (12, 12), None, "hamming"), ((0, 0, 40, 30), (60, 45), (20, 15, 30, 16), "nearest"), ((10, 10, 16, 16), (8, 8), None, "bilinear")],
                  [((0, 0, 9, 9), (27, 27), (20, 20, 7, 7), "bicubic"), ((1015, 0, 9, 1024), (3, 64), (0, 8, 3, 16), "bilinear"), ((512, 512, 96, 32), (48, 16), None, "bicubic")]]
PREMULTIPLIED_VIEW = ((200, 300, 90, 40), (70, 30), (2, 3, 65, 17), "lanczos")


@pytest.mark.parametrize("premultiplied", [False, True])
@pytest.mark.parametrize("layout", ["planar", "hwc"])
def test_resample_views_in_several_groups_around_a_file_without_a_job(enc, big_files, layout, premultiplied):  # noqa: F811
    """a RESAMPLE call over several groups: the launch kind, the LDS size and the alpha instantiation are picked per group from that
    group's records, and the NEAREST index tables are re-based per job next to a file that gets none.  premultiplied: file 2 has a
    PREMULTIPLIED Lanczos view more (the files are RGBA noise), so the groups differ in the alpha instantiation too.  Every view of
    files 0 and 2 equals the model of the reference decoder's planes and the same view decoded in a one-file call; file 1's
    destinations stay sentinel.  One sentinel-filled buffer per call, compared whole and bit for bit"""
    import torch
    kinds = _kinds(layout)
    per_file = [list(v) for v in RESAMPLE_VIEWS]
    alpha = [[NONE] * 3 for _ in per_file]
    if premultiplied:
        per_file[2].append(PREMULTIPLIED_VIEW)
        alpha[2].append(PRE)
    post = [[{}, {"blur": (2, 1.3)}, {}]] + [[{}] * len(v) for v in per_file[1:]]
    tone = [[{}, {}, EQUAL]] + [[{}] * len(v) for v in per_file[1:]]
    plan = [(3 + (i & 1), [(crop, full, window, f, bool((i + k) & 1), kinds[(i + k) % len(kinds)]) for k, (crop, full, window, f) in enumerate(vs)]) for i, vs in enumerate(per_file)]
    model = _Model(big_files)

    def decode(idx):
        stages = {"post": [post[i] for i in idx], "tone": [tone[i] for i in idx]}
        if premultiplied:
            stages["alpha"] = [alpha[i] for i in idx]
        sub = [plan[i] for i in idx]
        got, host, outs, regs = _decode(enc, layout, [big_files.pngs[i] for i in idx], sub, "uint8", False, **stages)
        want = _sources(model, idx, sub, "uint8", skip=[n for n, i in enumerate(idx) if i == 1], **stages)
        diff = _difference(layout, host, "uint8", regs, want)  # (None for file 1's views: all sentinel)
        assert diff is None, (layout, premultiplied, idx, diff)
        return [st for st, _, _ in got], [[t.cpu() for t in ts] for ts in outs]

    statuses, together = decode([0, 1, 2])
    assert statuses == [0, CROP_OUTSIDE, 0]
    assert all(bool((t == SENTINEL).all()) for t in together[1])
    for i in (0, 2):
        (st,), (alone,) = decode([i])
        assert st == 0 and len(alone) == len(together[i])
        for k, (a, b) in enumerate(zip(together[i], alone)):
            assert not bool((b == SENTINEL).all()) and torch.equal(a, b), (layout, i, k)
