"""GPU test of the views calls' record indexing across GROUPS of files when a file in the middle gets no job: three large stored
host files -- several groups -- whose middle file's crop leaves the image, the other two with a direct view, a blur view and a tone
view each.  Every view must be byte-equal to the same view decoded alone in a one-file call of the same entry point, and the middle
file's destinations stay untouched."""
import pytest

from test_gpu_decode_layouts import SENTINEL
from test_gpu_decode_resize import CROP_OUTSIDE, enc  # noqa: F401  (enc: a fixture)
from test_gpu_decode_views import big_files  # noqa: F401  (a fixture)

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
