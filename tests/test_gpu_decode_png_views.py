"""Views of ordinary PNG files on the GPU (-m gpu; fpng_amd_decode_batch(_device)_png_views, fpng_amd/csrc/png_views_api.cpp and
png_unfilter_box_kernel).  The oracle is code the project had before the call: decode_device_png of the file (4 channels when it
has an alpha plane, else 3), those pixels through the fpng encoder, and that file through the existing views calls; the new call
must give the same elements, torch.equal, in uint8 and in every float type.  One test ties a plain view to Pillow directly.  Every
file stays under about 100 KB of scanlines (130 x 130 and 200 x 150 at most): the inflate kernel works through about 5 MB of them
per second and wavefront."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest

import inflate_cases as ic
import png_views_cases as V

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


@pytest.fixture(scope="module")
def enc(built_lib):
    import torch
    import fpng_amd
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    e = fpng_amd.Encoder(device=0)
    yield e
    e.close()


KINDS = ("grey", "grey_alpha", "rgb", "rgba", "palette", "palette_trns", "grey_key", "rgb_key")


def _typed_files():
    """one file per colour type -- palette with and without tRNS, grey and RGB with a key -- written by Pillow, and two token-level
    files of inflate_cases.py (one row of one-byte pixels each)"""
    names, files, views = [], [], []
    for k, kind in enumerate(KINDS):
        w, h = (200, 150) if k % 3 == 1 else (130, 130)
        names.append(kind), files.append(V.pillow_file(kind, w, h, 100 + k)), views.append(V.three_views(w, h))
    cases = ic.accepted_cases()
    for c in (cases[len(cases) // 3], cases[-1]):
        w, h = c.dims
        assert h == 1 and w >= 2
        names.append(c.name), files.append(c.file)
        views.append([((0, 0, w, 1), ((w + 7) // 8, 1), None, "bilinear", False), ((w // 2, 0, min(64, w - w // 2), 1), (24, 3), None, "bicubic", True)])
    return names, files, views


def test_the_rule_for_alpha_planes_on_the_test_files():
    names, files, _ = _typed_files()
    assert [V.alpha_plane(f) for f in files[:8]] == [False, True, False, True, False, True, True, True]
    assert [f[25] for f in files[:8]] == [0, 4, 2, 6, 3, 3, 0, 2]
    for f in files:
        w, h = V.dims(f)
        assert h * (1 + w * 4) <= 130000


def test_same_elements_as_the_oracle_planar_uint8(enc):
    import torch
    names, files, views = _typed_files()
    got, _ = V.same_as_oracle(enc, files, views, [3] * len(files), torch.uint8, "planar", names)
    assert [c for _, _, c in got[:8]] == [1, 2, 3, 4, 3, 4, 1, 3]  # (channels_in_file: what decode_device_png reports)
    V.same_as_oracle(enc, files, views, [4 if V.alpha_plane(f) else 3 for f in files], torch.uint8, "planar", names)
    V.same_as_oracle(enc, files, views, [4] * len(files), torch.uint8, "planar", names)  # (a file without an alpha plane: 255)


def test_same_elements_as_the_oracle_planar_f16(enc):
    import torch
    names, files, views = _typed_files()
    V.same_as_oracle(enc, files, views, [3] * len(files), torch.float16, "planar", names, mean=MEAN, std=STD)
    V.same_as_oracle(enc, files, views, [3] * len(files), torch.float32, "planar", names, mean=MEAN, std=STD)


def test_same_elements_as_the_oracle_hwc_bf16(enc):
    import torch
    names, files, views = _typed_files()
    V.same_as_oracle(enc, files, views, [3] * len(files), torch.bfloat16, "hwc", names, mean=MEAN, std=STD)
    V.same_as_oracle(enc, files, views, [4 if V.alpha_plane(f) else 3 for f in files], torch.uint8, "hwc", names)


def test_a_plain_bilinear_view_is_pillows(enc):
    """Image.open(f).convert("RGB").crop(box).resize(size, BILINEAR), byte for byte, for an RGB and a palette file"""
    import torch
    from PIL import Image
    for kind in ("rgb", "palette"):
        f = V.pillow_file(kind, 130, 130, 7)
        box, size = (5, 7, 120, 118), (56, 48)
        res, outs = V.run(enc, [f], [[(box, size, None, "bilinear", False)]], [3], torch.uint8, "planar")
        assert res[0][0] == 0
        with Image.open(io.BytesIO(f)) as im:
            want = np.asarray(im.convert("RGB").crop((box[0], box[1], box[0] + box[2], box[1] + box[3])).resize(size, Image.BILINEAR))
        assert np.array_equal(outs[0][0].cpu().numpy().transpose(1, 2, 0), want), kind


def test_stages(enc):
    """one batch of four files through colour matrices, a blur, a rotate warp, autocontrast, sharpness, a composite alpha record on
    the RGBA and the palette + tRNS file (4-plane and 3-plane destinations) and a NEAREST resample on a palette "mask": the oracle's"""
    import torch
    import fpng_amd
    w = h = 130
    names = ["rgb", "rgba", "palette_trns", "mask"]
    files = [V.pillow_file(k, w, h, 200 + i) for i, k in enumerate(names)]
    views = [[((5, 7, 120, 118), (56, 56), None, "bilinear", False), ((64, 64, 40, 40), (48, 40), None, "bicubic", True)] for _ in files]
    none_post, none_warp, none_tone, none_enh, none_alpha = fpng_amd.view_post(), fpng_amd.view_warp(), fpng_amd.view_tone(), fpng_amd.view_enhance(), fpng_amd.view_alpha()
    blur, rot = fpng_amd.view_post(blur=(5, 1.1)), fpng_amd.view_warp(fpng_amd.rotate_matrix(56, 56, 15.0), "bilinear", (1, 2, 3))
    comp = fpng_amd.view_alpha("composite", (255, 200, 10))
    stages = dict(color=fpng_amd.color_matrix(brightness=1.1, contrast=0.9, saturation=0.8),
                  post=[[blur, none_post], [none_post, blur], [blur, none_post], [none_post, none_post]],
                  warp=[[rot, none_warp], [rot, none_warp], [none_warp, none_warp], [rot, none_warp]],
                  tone=[[fpng_amd.view_tone(autocontrast=True), none_tone], [none_tone, none_tone], [none_tone, fpng_amd.view_tone(autocontrast=True)], [none_tone, none_tone]],
                  enhance=[[none_enh, fpng_amd.view_enhance(sharpness=1.7)], [fpng_amd.view_enhance(sharpness=0.4), none_enh], [none_enh, none_enh], [none_enh, none_enh]],
                  alpha=[[none_alpha, none_alpha], [comp, none_alpha], [comp, comp], [none_alpha, none_alpha]],
                  resample=[[None, None], [None, "box"], [None, None], ["nearest", "nearest"]])
    chans = [3, 4, 3, 3]
    V.same_as_oracle(enc, files, views, chans, torch.uint8, "planar", names, **stages)
    V.same_as_oracle(enc, files, views, chans, torch.float16, "hwc", names, mean=MEAN, std=STD, **stages)


def _check_routing(enc, flags):
    import torch
    names, files, views, want = V.routing_batch(enc)
    chans = [3] * len(files)
    res, outs = V.run(enc, files, views, chans, torch.uint8, "planar", flags=flags)
    plain = enc.decode_device_png(V.to_device(files), 3, flags=flags)
    good = [i for i in range(len(files)) if want[i] == 0]
    ores, oouts = V.run(enc, [V.oracle_file(enc, files[i]) for i in good], [views[i] for i in good], [3] * len(good), torch.uint8, "planar", png=False)
    seen = set()
    for i, name in enumerate(names):
        st = res[i][0]
        seen.add(st)
        if want[i] is None:  # (a damaged file: the status decode_device_png gives it)
            assert st == plain[i][0] != 0, name
        else:
            assert st == want[i], (name, st)
        if st:
            assert res[i][1] is None and all(V.untouched(t) for t in outs[i]), name  # (a failed file: none of its views is written)
        else:
            k = good.index(i)
            assert ores[k][0] == 0 and all(torch.equal(a, b) for a, b in zip(outs[i], oouts[k])), name
            assert res[i][2] == plain[i][2], name
    assert {0, 67, 68} <= seen and len(seen) >= 4
    return [[o.cpu().numpy() for o in os_] for os_ in outs]


def test_routing(enc):
    """statuses per file; the views of the files that succeed equal their oracles'; the destinations of failed files are untouched;
    FPNG_AMD_PNG_GENERAL_ONLY gives the same elements, the fpng-written files included"""
    import fpng_amd
    routed = _check_routing(enc, 0)
    general = _check_routing(enc, fpng_amd.FPNG_AMD_PNG_GENERAL_ONLY)
    for a, b in zip(routed, general):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_groups_give_the_same_elements():
    """FPNG_AMD_PNG_SCRATCH_LIMIT, set in a fresh child process, so small that every file is a group of its own: the same statuses and
    elements as in one group, post and tone views included (png_views_cases.py is the child)"""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.path.join(ROOT, "tests"))
    env.pop("FPNG_AMD_PNG_SCRATCH_LIMIT", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "png_views_cases.py")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().startswith("OK"), (r.stdout[-500:], r.stderr[-3000:])


def test_two_groups_with_the_undecided_file_in_the_second():
    """a mixed batch of files of at most 129 x 65, routed, with FPNG_AMD_PNG_SCRATCH_LIMIT computed from the per-file terms so that
    exactly two groups form and the fpng-written file that the fpng path leaves UNDECIDED (tests/golden/first_pixel_match.png) comes
    to the tier behind the files routed at once, in the second group: the statuses and elements of the one-group run"""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.path.join(ROOT, "tests"))
    env.pop("FPNG_AMD_PNG_SCRATCH_LIMIT", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "png_views_cases.py"), "two"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().startswith("OK"), (r.stdout[-500:], r.stderr[-3000:])


def test_host_resident_files_equal_the_device_form(enc):
    import torch
    names, files, views, want = V.routing_batch(enc)
    chans = [3] * len(files)
    dev, douts = V.run(enc, files, views, chans, torch.float16, "hwc", mean=MEAN, std=STD)
    host, houts = V.run(enc, files, views, chans, torch.float16, "hwc", host=True, mean=MEAN, std=STD)
    for name, a, b, x, y in zip(names, dev, host, douts, houts):
        assert a[0] == b[0] and a[2] == b[2], name
        assert all(torch.equal(p, q) for p, q in zip(x, y)), name
    assert sum(1 for a in host if a[0] == 0) >= 6


def test_a_refused_call_launches_nothing(enc):
    """one destination of the last file is one byte short: FPNG_AMD_ERR_BUFFER_TOO_SMALL, and every destination of every file still
    holds its pattern"""
    import torch
    import fpng_amd
    names, files, views, _ = V.routing_batch(enc)
    keep = [i for i, n in enumerate(names) if n in ("fpng_rgb", "pillow_rgb", "pillow_palette_trns", "pillow_grey_alpha")]
    files, views = [files[i] for i in keep], [views[i] for i in keep]
    outs = [V.make_outs(v, 3, torch.uint8, "planar") for v in views]
    db = enc.make_decode_batch_png_views(V.to_device(files), [[v[0] for v in vs] for vs in views], outs, [[v[1] for v in vs] for vs in views],
                                         [[v[2] for v in vs] for vs in views], [[v[3] for v in vs] for vs in views], [[v[4] for v in vs] for vs in views])
    db.dests[len(db.dests) - 1].pixels_cap -= 1
    with pytest.raises(fpng_amd.FpngAmdError) as err:
        enc.decode_device_png_views(db)
    assert err.value.code == -4  # FPNG_AMD_ERR_BUFFER_TOO_SMALL
    torch.cuda.synchronize()
    assert all(V.untouched(t) for ts in outs for t in ts)
    db.dests[len(db.dests) - 1].pixels_cap += 1  # (the same descriptor, made good: it runs)
    res = enc.decode_device_png_views(db)
    assert [st for st, _, _ in res] == [0] * len(files) and not any(V.untouched(t) for ts in outs for t in ts)
