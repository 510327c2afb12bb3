"""GPU decoder of views with EVERY stage's array given in one call (-m gpu; the _views_resample calls with alpha=, resample=, color=,
post=, warp=, tone= and enhance= at once): each of the six filters -- Pillow's nearest, box, Hamming and Lanczos through their
records, bilinear and bicubic as the views' own -- followed at least once by each of solarize, posterize, a blur, a warp that moves,
equalize or autocontrast, and an enhance op; one view with all stages at once (PREMULTIPLIED, Lanczos, a matrix, a warp, a tone op,
an enhance op, a blur) and one with none, which is a direct view in a post call.  The RGBA pattern file and the 3-channel noise
file, windows of at most 65 x 17, uint8 and a float dtype, both layouts.

Expected values never come from the library: the bytes are the REFERENCE's decoder's, through resample_model.py and
alpha_model.view_elements with all ten arguments filled.  Every call decodes into ONE sentinel-filled buffer that is compared
WHOLE and bit for bit."""
import pytest

from test_gpu_decode_float import CONSTS
from test_gpu_decode_resize import enc  # noqa: F401  (enc: a fixture)
from test_gpu_decode_views_color import LAYOUTS, _matrices
from test_gpu_decode_views_resample import NOISE, RGBA, rfiles, rmodel  # noqa: F401  (rfiles, rmodel: fixtures)
from test_gpu_decode_views_resample_alpha import NONE, PRE, TEAL, _check_conditions, _kinds, _run
from test_gpu_decode_views_tone import AUTO, EQUAL
from test_gpu_decode_views_warp import _matrix
from test_gpu_resize_view import _window
from test_views_color_cpu import IDENTITY
import resample_model as SM  # (before any model is asked for a new filter's name)
import resize_view_model as VM

pytestmark = pytest.mark.gpu

FILTERS = SM.NEW_FILTERS + VM.FILTERS
FOLLOWERS = ("solarize", "posterize", "blur", "warp", "tone", "enhance")
# (crop, full, window): windows of at most 65 x 17; shrunk in x and grown in y, the far corner, an upscale, a crop inside the file
SHAPES = [((0, 0, 600, 130), (224, 224), (150, 200, 64, 16)), ((0, 0, 600, 130), (300, 65), (235, 48, 65, 17)), ((5, 7, 9, 11), (65, 17), None), ((100, 10, 450, 100), (150, 33), (85, 16, 65, 17)),
          ((300, 40, 300, 90), (112, 112), (3, 50, 33, 9))]
ENHANCE = ({"brightness": 1.4}, {"color": 0.4}, {"sharpness": 2.0})


def _follower(name, n, shape):
    """-> (post, warp, tone, enhance) records of a view whose resize is followed by `name` alone"""
    w, h = _window(shape[1], shape[2])[2:]
    post, warp, tone, enhance = {}, {}, {}, {}
    if name == "solarize":
        post = {"solarize": (100, 128, 200)[n % 3]}
    elif name == "posterize":
        post = {"posterize": (3, 5)[n % 2]}
    elif name == "blur":
        post = {"blur": ((1, 0.8), (2, 1.0), (4, 2.0))[n % 3]}
    elif name == "warp":
        warp = {"a": _matrix((0, 0, w, h), angle=(20.0, -35.0)[n % 2], translate=(1.5, -0.75)), "filter": ("nearest", "bilinear")[n % 2], "fill": (10 + n, 20, 230, 40)}
    elif name == "tone":
        tone = (EQUAL, AUTO)[n % 2]
    else:
        enhance = ENHANCE[n % 3]
    return post, warp, tone, enhance


def _plan(layout, flip):
    """two files, the RGBA pattern and the 3-channel noise: view (filter a, follower b) goes to file (a + b) % 2 under shape
    (2 a + b) % 5; on the RGBA file the alpha ops go round (NEAREST takes no PREMULTIPLIED record: a COMPOSITE instead), on the
    3-channel file every op is the identity and some views carry one all the same; every other view has a real matrix; then the view
    with every stage and the view with none.  -> idx, plan, stages"""
    kinds = _kinds(layout)
    plan = [(4 - flip, []), (3 + flip, [])]
    stages = {k: [[], []] for k in ("alpha", "post", "warp", "tone", "enhance")}
    real = [[], []]  # (per view: whether its matrix is a real one)
    met = set()

    def add(n, shape, f, alpha, post, warp, tone, enhance, matrix):
        k = len(plan[n][1])
        plan[n][1].append((shape[0], shape[1], shape[2], f, flip ^ bool(k & 1), kinds[(k + n + flip) % len(kinds)]))
        for name, rec in (("alpha", alpha), ("post", post), ("warp", warp), ("tone", tone), ("enhance", enhance)):
            stages[name][n].append(rec)
        real[n].append(matrix)

    for a, f in enumerate(FILTERS):
        for b, name in enumerate(FOLLOWERS):
            n, shape = (a + b) % 2, SHAPES[(2 * a + b) % len(SHAPES)]
            alpha = (PRE, TEAL, NONE)[(a + 2 * b) % 3]
            if f == "nearest" and alpha == PRE:
                alpha = TEAL
            add(n, shape, f, alpha, *_follower(name, a + b, shape), matrix=bool((a + b // 2) & 1))
            met.add((f, name))
    assert met == {(f, name) for f in FILTERS for name in FOLLOWERS}
    every = SHAPES[0]
    add(0, every, "lanczos", PRE, {"blur": (2, 1.2)}, _follower("warp", 1, every)[1], EQUAL, {"sharpness": 1.8}, matrix=True)
    add(0, SHAPES[1], "bilinear", NONE, {}, {}, {}, {}, matrix=False)
    add(1, SHAPES[3], "bicubic", NONE, {}, {}, {}, {}, matrix=False)
    seeded = _matrices(plan, 1300 + flip)
    stages["color"] = [[m if r else IDENTITY for m, r in zip(ms, rs)] for ms, rs in zip(seeded, real)]
    assert all(_window(full, window)[2] <= 65 and _window(full, window)[3] <= 17 for _, views in plan for _, full, window, *_ in views)
    return [RGBA, NOISE], plan, stages


@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_filter_in_front_of_every_later_stage(enc, rfiles, rmodel, layout):  # noqa: F811
    """the batch of _plan: uint8 from host files, and flipped (three and four planes swapped, every mirror flag) as float16 from device
    files"""
    assert rfiles.chans[RGBA] == 4 and rfiles.chans[NOISE] == 3
    crop, full, _ = SHAPES[0]  # (the view with every stage: its PREMULTIPLIED Lanczos resize clips in U and meets a colour under alpha 0)
    _check_conditions(rfiles, [(RGBA, crop, full)], "lanczos")
    for flip, dtype in ((False, "uint8"), (True, "float16")):
        idx, plan, stages = _plan(layout, flip)
        _run(enc, rfiles, rmodel, layout, idx, plan, dtype, flip, consts=CONSTS[flip], **stages)
