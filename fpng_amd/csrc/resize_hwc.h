// resize_hwc.h -- the second stage of fpng_amd_decode_batch(_device)_hwc_views (include/fpng_amd.h): the views call's resize with
// CHANNELS-LAST destinations.  The rule of the resize is resize.h's, untouched; what differs is who writes what: one workgroup of
// dec_resize_hwc_kernel (resize.hip) produces ALL planes of a tile of kResizeTileW x kResizeTileH window samples and writes whole
// pixels as contiguous runs, where dec_resize_exact_kernel runs a workgroup per plane.
#pragma once
#include "decode.h"
#include "resize.h"

namespace fpng_amd {

constexpr uint32_t kHwcReversed = 1u; // FPNG_AMD_HWC_REVERSED

// a view's work for dec_resize_hwc_kernel.  r: the planar record of the same view (source box, window, weights' sizes, mirror flag,
// filter, planes = num_chans) with r.dst = pixel (0, 0) of the view's top row, r.pitch = the signed bytes between rows and
// r.plane_pitch not used.  pixel_elems: elements from one pixel to the next (planes, or 4 with planes = 3: the fourth is never
// written); hwc_flags: kHwcReversed -- file channel c is element planes - 1 - c of its pixel
struct DecResizeHwc {
    DecResize r;
    uint32_t pixel_elems, hwc_flags;
};
static_assert(sizeof(DecResizeHwc) == 120 && offsetof(DecResizeHwc, r) == 0 && offsetof(DecResizeHwc, pixel_elems) == 112 && offsetof(DecResizeHwc, hwc_flags) == 116, "DecResizeHwc layout");

// the LDS bytes of one tile: resize_tile_lds(), whose bytes the tile's result bytes O[row][column * planes + plane] take over once
// the passes are done (a tile of few taps and rows needs less than O does)
FPNG_RESIZE_FN uint32_t resize_hwc_tile_lds(uint32_t taps_x, uint32_t taps_y, uint32_t rows, uint32_t planes)
{
    const uint32_t passes = resize_tile_lds(taps_x, taps_y, rows), o = kResizeTileH * kResizeTileW * planes;
    return passes > o ? passes : o;
}

// An exact grid as launch_dec_resize_exact's, a workgroup per (record, tile): pre (device) and h_pre (host, the same words) hold n + 1
// entries, the TILES of the batch's records in front of each of recs[0 .. n].  lds_bytes: the most resize_hwc_tile_lds() of the
// launch's records.  false: a record without or with too many tiles, or lds_bytes out of range; nothing is launched.
// any_alpha: some record of the launch carries an alpha op (view_alpha.h): the kernel's alpha instantiation.
bool launch_dec_resize_hwc(hipStream_t s, const DecResizeHwc *recs, const uint64_t *pre, const uint64_t *h_pre, uint32_t n, uint32_t lds_bytes, const DecFloat *flt, uint32_t filters,
                           bool any_alpha = false);

} // namespace fpng_amd
