"""The shapes of test_gpu_resize_limits.py, kept apart from it so that test_resize_bounds_cpu.py can sweep the host's bounds over the
same axes without importing a GPU test: full 64 x 16 tiles at and just under the scale limits (in <= 32 * out bilinear, 16 * out
bicubic), the record that splits a rectangular launch, and the tiny views that fill a batch of 600 files."""

LIMIT_FILE = (2080, 768)  # the smallest source that at 32 x gives a full 64-column tile plus a second tile column (65 columns) and a
#                           full 16-row tile plus a second tile row at a window that does not start on a tile boundary (24 rows)

# (crop, full, window or None, filter) of a 2080 x 768 file
LIMIT_VIEWS = [
    ((0, 0, 2080, 768), (65, 24), None, "bilinear"),             # exactly 32 x in both axes; tiles 64 x 16, 1 x 16, 64 x 8, 1 x 8
    ((0, 0, 2080, 768), (65, 24), (0, 7, 65, 17), "bilinear"),   # a tile that starts at row 7 of the full image and is full; the last one is a single row
    ((3, 5, 2075, 761), (65, 24), (1, 3, 64, 21), "bilinear"),   # 31.92 x / 31.71 x, not an integer
    ((0, 0, 1040, 384), (65, 24), None, "bicubic"),              # exactly 16 x
    ((0, 0, 1040, 384), (65, 24), (0, 7, 65, 17), "bicubic"),
    ((3, 5, 1037, 381), (65, 24), None, "bicubic"),              # just under the bicubic limit
    ((0, 0, 96, 768), (3, 24), None, "bilinear"),                # the 32 x rows with three columns
    ((0, 0, 2080, 64), (65, 2), None, "bilinear"),               # 65 taps across a full tile row with two rows
    ((0, 0, 64, 768), (128, 24), None, "bilinear"),              # x grows while y is at the limit: the launch's LDS is decided by rows alone
    ((7, 9, 9, 11), (65, 17), None, "bilinear"),                 # small upscales in the same call: the launch's LDS (its maximum) is far
    ((7, 9, 9, 11), (65, 17), None, "bicubic"),                  # above these records' own layout
]

# ---- the batch of 600 files ----
SPLIT_FILES = 600
SPLIT_AT = 590                              # the large record's index: in the second launch, while the first one's grid is sized by it
SPLIT_CROP, SPLIT_SIZE = (0, 0, 600, 130), (4096, 1792)  # 64 x 112 = 7168 tiles of 64 x 16
MANY_FULL, MANY_WINDOW = (300, 65), (0, 0, 129, 33)      # the exact grid's large view: three tile columns and rows, the last ones partial


def split_step(max_tiles):
    """records per launch of a rectangular grid of (max_tiles, 4 planes, records) workgroups of 256 threads: fewer than 2^32 threads a
    launch, at most 32768 records (the rule of launch_dec_resize, restated from its constants)"""
    return min(32768, ((1 << 32) - 1) // (max_tiles * 4 * 256))


def tiny_view(k, dims):
    """(crop, (out_w, out_h)) of tiny file k, a 1 x 1 or a 64 x 97 one: outputs 1 x 1 .. 5 x 5, the crop inside both filters' limits"""
    s = 1 + k % 5
    if dims == (1, 1):
        return (0, 0, 1, 1), (s, s)
    assert dims == (64, 97)
    return (k % 7, k % 11, min(16 * s, 57), min(16 * s, 86)), (s, s)


def axis_pairs():
    """every (filter, in, out) of one axis that the GPU tests resize with"""
    pairs = set()
    for crop, full, _, f in LIMIT_VIEWS:
        pairs |= {(f, crop[2], full[0]), (f, crop[3], full[1])}
    for f in ("bilinear", "bicubic"):
        pairs |= {(f, SPLIT_CROP[2], MANY_FULL[0]), (f, SPLIT_CROP[3], MANY_FULL[1])}
        for k in range(35):  # (5 sizes x 7 x 11 origins: the crop's size depends on k % 5 alone)
            for dims in ((1, 1), (64, 97)):
                crop, size = tiny_view(k, dims)
                pairs |= {(f, crop[2], size[0]), (f, crop[3], size[1])}
    pairs |= {("bilinear", SPLIT_CROP[2], SPLIT_SIZE[0]), ("bilinear", SPLIT_CROP[3], SPLIT_SIZE[1])}
    return pairs
