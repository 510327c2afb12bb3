"""No-GPU test of the ORDER in which the 24 views entry points -- fpng_amd_decode_batch(_device)_{planar,hwc}_views and their _color,
_post, _warp, _tone and _enhance siblings -- test their refusals.  Every call gets a NULL encoder and two files with 2 + 1 views (the
records of the other _cpu tests); a case spoils that good set in one or in two places, and the call's return code and the exact text of
fpng_amd_last_error() are compared with literals: a single NULL pointer in turn, pairs of faults that different layers of the host
code judge (which one is reported is the order under test), and the good set, which only the missing encoder stops."""
import ctypes as C

import pytest

from fpng_amd import _lib

from test_resize_view_cpu import GOOD
from test_views_post_cpu import _arrays

STAGES = ("colors", "posts", "warps", "tones", "enhances")  # the record arrays a family's call takes, in its argument order
FAMILIES = ("", "_color", "_post", "_warp", "_tone", "_enhance")  # family k takes STAGES[:k]
NAMES = [f"fpng_amd_decode_batch{dev}_{layout}_views{fam}" for layout in ("planar", "hwc") for fam in FAMILIES for dev in ("", "_device")]
NAN = float("nan")


def _good(hwc):
    """the good set by argument name (fmt: float32, so that an element has 4 bytes)"""
    files, cnt, c, v, d, col, post, res = _arrays([GOOD[0], GOOD[1], GOOD[2]], [2, 1], hwc)
    return {"files": files, "view_count": cnt, "crops": c, "views": v, "dests": d, "colors": col, "posts": post, "warps": (_lib.ViewWarp * 3)(),
            "tones": (_lib.ViewTone * 3)(), "enhances": (_lib.ViewEnhance * 3)(), "fmt": _lib.FloatFormat(), "results": res}


def _set(arg, index, **fields):
    def spoil(a):
        for name, value in fields.items():
            setattr(a[arg][index], name, value)
    return {arg}, spoil


def _null(arg):
    return {arg}, lambda a: a.__setitem__(arg, None)


def _nan_matrix(a):
    a["colors"][2].m[1][1] = NAN


# fault -> (the arguments it needs, what it does to the good set); *_hwc: channels-last calls only
FAULTS = {f"null_{arg}": _null(arg) for arg in ("files", "view_count", "crops", "views", "dests", *STAGES, "fmt", "results")}
FAULTS.update({
    "bad_post": _set("posts", 1, flags=8), "wide_blur": _set("posts", 1, flags=_lib.POST_BLUR, blur_radius=4, blur_sigma=1.0),  # (view 1: 6 x 4)
    "bad_warp": _set("warps", 1, flags=4), "bad_tone": _set("tones", 1, op=4), "bad_enhance": _set("enhances", 2, op=4),
    "bad_color": ({"colors"}, _nan_matrix), "count_0": ({"view_count"}, lambda a: a["view_count"].__setitem__(1, 0)),
    "file_d_pixels": _set("files", 0, d_pixels=256), "bad_chans": _set("files", 1, num_chans=5), "bad_filter": _set("views", 1, filter=2),
    "misaligned": _set("dests", 0, d_pixels=2), "wide_pitch": _set("dests", 2, row_pitch=1 << 31),
    "bad_dtype": ({"fmt"}, lambda a: setattr(a["fmt"], "dtype", 7)),
    "bad_pixel_elems_hwc": _set("dests", 1, pixel_elems=5), "bad_flags_hwc": _set("dests", 2, flags=2)})

SINGLES = [(f,) for f in FAULTS]
# two faults at once, judged by different layers of the host code
PAIRS = [("null_enhances", "bad_post"), ("bad_tone", "count_0"), ("bad_color", "file_d_pixels"), ("bad_pixel_elems_hwc", "misaligned"),
         ("null_enhances", "null_dests"), ("null_tones", "bad_enhance"), ("null_warps", "bad_tone"), ("null_posts", "bad_color"), ("null_posts", "null_dests"),
         ("null_colors", "bad_post"), ("null_colors", "null_dests"), ("null_colors", "null_view_count"), ("null_dests", "bad_color"), ("null_dests", "bad_enhance"),
         ("bad_enhance", "bad_tone"), ("bad_tone", "bad_warp"), ("bad_warp", "bad_post"), ("bad_post", "bad_color"), ("bad_color", "bad_filter"),
         ("bad_color", "count_0"), ("bad_color", "null_files"), ("bad_color", "null_results"), ("bad_enhance", "null_files"), ("wide_blur", "null_views"),
         ("bad_filter", "file_d_pixels"), ("file_d_pixels", "bad_pixel_elems_hwc"), ("bad_flags_hwc", "bad_dtype"), ("bad_dtype", "bad_chans"),
         ("bad_chans", "misaligned"), ("misaligned", "wide_pitch"), ("bad_pixel_elems_hwc", "bad_chans"), ("null_view_count", "bad_tone"),
         ("null_view_count", "null_files"), ("null_crops", "bad_post"), ("bad_filter", "null_results"), ("bad_dtype", "null_files")]
CASES = [()] + SINGLES + PAIRS

# The return code is -1 (FPNG_AMD_ERR_INVALID_ARG) in every case.  case -> the text, or "layout family" -> text where the calls differ
# ("*": every call the case applies to that is not listed)
NO_ENCODER = "null/empty batch"
NULL_ARRAY = "null files, view_count, crops, views, dests or results"
BAD_POST = "unknown fpng_amd_view_post::flags bits (FPNG_AMD_POST_BLUR, _SOLARIZE, _POSTERIZE)"
BAD_WARP = "unknown fpng_amd_view_warp::flags bits (FPNG_AMD_WARP_AFFINE, _BILINEAR)"
BAD_TONE = "unknown fpng_amd_view_tone::op (FPNG_AMD_TONE_AUTOCONTRAST, _EQUALIZE, _CONTRAST)"
BAD_ENHANCE = "unknown fpng_amd_view_enhance::op (FPNG_AMD_ENHANCE_BRIGHTNESS, _COLOR, _SHARPNESS)"
BAD_COLOR = "fpng_amd_view_color::m: every entry must be finite and at most 65536 in magnitude"
COUNT_0 = "a view_count of 0 (every file has at least one view)"
FILE_DEST = "fpng_amd_png_planar::d_pixels, row_pitch, plane_pitch and pixels_cap must be NULL / 0: the destinations are the fpng_amd_view_dest records"
BAD_FILTER = "unknown filter (FPNG_AMD_FILTER_BILINEAR, _BICUBIC)"
BAD_PIXEL_ELEMS = "fpng_amd_view_dest_hwc::pixel_elems must be 0, num_chans, or 4 with num_chans = 3"
BAD_HWC_FLAGS = "unknown fpng_amd_view_dest_hwc::flags bits"
EXPECTED = {
    "": NO_ENCODER,
    "null_files": NULL_ARRAY, "null_view_count": NULL_ARRAY, "null_crops": NULL_ARRAY, "null_views": NULL_ARRAY, "null_dests": NULL_ARRAY, "null_results": NULL_ARRAY,
    "null_colors": {"planar _color": "null colors", "hwc _color": "null colors", "*": NO_ENCODER},  # (behind the colour call NULL is the identity, ...
    "null_posts": {"planar _post": "null posts", "hwc _post": "null posts", "*": NO_ENCODER},       #  ... no flags, ...
    "null_warps": {"planar _warp": "null warps", "hwc _warp": "null warps", "*": NO_ENCODER},       #  ... no warp, ...
    "null_tones": {"planar _enhance": NO_ENCODER, "hwc _enhance": NO_ENCODER, "*": "null tones"},   #  ... no op)
    "null_enhances": "null enhances", "null_fmt": NO_ENCODER,
    "bad_post": BAD_POST, "wide_blur": "fpng_amd_view_post::blur_radius must be below the window's w and h (one reflection at the border)",
    "bad_warp": BAD_WARP, "bad_tone": BAD_TONE, "bad_enhance": BAD_ENHANCE, "bad_color": BAD_COLOR, "count_0": COUNT_0, "file_d_pixels": FILE_DEST,
    "bad_filter": BAD_FILTER, "bad_pixel_elems_hwc": BAD_PIXEL_ELEMS, "bad_flags_hwc": BAD_HWC_FLAGS,
    # (the element type, the channel count, the destinations' alignment and pitch: judged behind the encoder)
    "bad_chans": NO_ENCODER, "misaligned": NO_ENCODER, "wide_pitch": NO_ENCODER, "bad_dtype": NO_ENCODER,
    "null_enhances + bad_post": "null enhances", "bad_tone + count_0": COUNT_0, "bad_color + file_d_pixels": BAD_COLOR, "bad_pixel_elems_hwc + misaligned": BAD_PIXEL_ELEMS,
    "null_enhances + null_dests": "null enhances", "null_tones + bad_enhance": BAD_ENHANCE, "null_warps + bad_tone": BAD_TONE,
    "null_posts + bad_color": {"planar _post": "null posts", "hwc _post": "null posts", "*": BAD_COLOR},
    "null_posts + null_dests": {"planar _post": "null posts", "hwc _post": "null posts", "*": NULL_ARRAY},
    "null_colors + bad_post": BAD_POST,
    "null_colors + null_dests": {"planar _color": "null colors", "hwc _color": "null colors", "*": NULL_ARRAY},
    "null_colors + null_view_count": {"planar _color": "null colors", "hwc _color": "null colors", "*": NULL_ARRAY},
    "null_dests + bad_color": NULL_ARRAY, "null_dests + bad_enhance": NULL_ARRAY, "bad_enhance + bad_tone": BAD_ENHANCE, "bad_tone + bad_warp": BAD_TONE,
    "bad_warp + bad_post": BAD_WARP, "bad_post + bad_color": BAD_POST, "bad_color + bad_filter": BAD_COLOR, "bad_color + count_0": COUNT_0,
    "bad_color + null_files": BAD_COLOR, "bad_color + null_results": BAD_COLOR, "bad_enhance + null_files": BAD_ENHANCE, "wide_blur + null_views": NULL_ARRAY,
    "bad_filter + file_d_pixels": BAD_FILTER, "file_d_pixels + bad_pixel_elems_hwc": FILE_DEST, "bad_flags_hwc + bad_dtype": BAD_HWC_FLAGS,
    "bad_dtype + bad_chans": NO_ENCODER, "bad_chans + misaligned": NO_ENCODER, "misaligned + wide_pitch": NO_ENCODER, "bad_pixel_elems_hwc + bad_chans": BAD_PIXEL_ELEMS,
    "null_view_count + bad_tone": NULL_ARRAY, "null_view_count + null_files": NULL_ARRAY, "null_crops + bad_post": BAD_POST, "bad_filter + null_results": NULL_ARRAY,
    "bad_dtype + null_files": NULL_ARRAY}


def _applies(case, layout, k):
    args = {"files", "view_count", "crops", "views", "dests", "fmt", "results", *STAGES[:k]}
    return all(FAULTS[f][0] <= args and (layout == "hwc" or not f.endswith("_hwc")) for f in case)


def observe(name, case):
    """(return code, message) of entry point `name` for the good set spoiled by `case`, or None where the case does not apply"""
    layout = "hwc" if "_hwc_" in name else "planar"
    k = FAMILIES.index(name[name.index("_views") + len("_views"):])
    if not _applies(case, layout, k):
        return None
    lib = _lib.load()
    a = _good(layout == "hwc")
    for f in case:
        FAULTS[f][1](a)
    fmt = C.byref(a["fmt"]) if a["fmt"] is not None else None
    rc = getattr(lib, name)(None, a["files"], 2, a["view_count"], a["crops"], a["views"], a["dests"], *[a[s] for s in STAGES[:k]], fmt, a["results"])
    return rc, lib.fpng_amd_last_error().decode()


def expected(name, case):
    e = EXPECTED[" + ".join(case)]
    if isinstance(e, str):
        return e
    layout = "hwc" if "_hwc_" in name else "planar"
    return e.get(f"{layout} {name[name.index('_views') + len('_views'):]}".rstrip(), e.get("*"))


@pytest.mark.parametrize("name", NAMES)
def test_refusal_precedence(built_lib, name):
    ran = 0
    for case in CASES:
        got = observe(name, case)
        if got is None:
            continue
        assert got == (-1, expected(name, case)), (name, case, got)
        ran += 1
    assert ran >= 20 and observe(name, ()) == (-1, "null/empty batch")
