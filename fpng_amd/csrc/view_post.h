// view_post.h -- the third stage of fpng_amd_decode_batch(_device)_planar_views_post and _hwc_views_post (include/fpng_amd.h): what
// contrastive recipes put behind the colour step -- a Gaussian blur, solarize and posterize, drawn per view -- on the BYTES that the
// colour call writes for the view's un-mirrored window.  The rule's pieces are the ONE text below, run by dec_view_post_kernel
// (view_post.hip) for every element and by the host function fpng_amd_view_post_apply (decode_api.cpp) that the CPU tests judge
// against an exact restatement.
//
//   B: the window's bytes, (uint8_t)rintf(u_c) of the colour rule, w x h per plane.  Planes 0, 1, 2 only: a fourth one skips all of this.
//   blur (radius R >= 1): the weights k[0 .. R] come from the HOST (post_blur_weights: exp in IEEE double; the kernel never evaluates
//       exp); tap t = -R .. R has weight k[|t|]; two passes, both to bytes, each the resize's pass (resize.h: resize_clip8):
//           H[q][i] = clip8(2^21 + sum_t B[q][refl(i + t, w)] * k[|t|])
//           G[q][i] = clip8(2^21 + sum_t H[refl(q + t, h)][i] * k[|t|])
//       refl(j, n) = j < 0 ? -j : j >= n ? 2 (n - 1) - j : j: the border reflects without repeating the edge, and with R < min(w, h)
//       (the host refuses anything else) one reflection lands inside.  The weights are not negative and sum to 2^22 give or take R
//       units, so a sum stays below 2^31 and its order is free.  Without blur G = B.
//   solarize:  S = G >= threshold ? 255 - G : G
//   posterize: Z = S & (0xFF00 >> bits) & 0xFF            8 is the identity, 0 gives 0
#pragma once
#include "decode.h"
#include "exact_grid.h"
#include "resize.h"
#include "view_enhance.h"
#include "view_tone.h"
#include "view_warp.h"

#include <cmath>

namespace fpng_amd {

constexpr uint32_t kPostBlur = 1u, kPostSolarize = 2u, kPostPosterize = 4u; // FPNG_AMD_POST_*
constexpr uint32_t kPostMaxRadius = 16;                                     // FPNG_AMD_BLUR_MAX_RADIUS

FPNG_RESIZE_FN uint32_t post_refl(int32_t j, uint32_t n) { return j < 0 ? (uint32_t)-j : (uint32_t)j >= n ? 2u * (n - 1u) - (uint32_t)j : (uint32_t)j; }

// steps 3 and 4 for one byte g of a view whose record has `flags`
FPNG_RESIZE_FN uint32_t post_point(uint32_t g, uint32_t flags, uint32_t threshold, uint32_t bits)
{
    if ((flags & kPostSolarize) && g >= threshold) g = 255u - g;
    if (flags & kPostPosterize) g &= (0xFF00u >> bits) & 0xFFu;
    return g;
}

// the weights of radius R (1 .. kPostMaxRadius) and sigma (finite, > 0): k[d], d = 0 .. R; the rest 0.  Host only.
inline void post_blur_weights(uint32_t radius, double sigma, int32_t k[kPostMaxRadius + 1])
{
#pragma clang fp contract(off)
    double p[kPostMaxRadius + 1];
    for (uint32_t d = 0; d <= radius; d++) p[d] = std::exp(-0.5 * ((double)d / sigma) * ((double)d / sigma));
    double ww = p[0];
    for (uint32_t d = 1; d <= radius; d++) ww = ww + 2.0 * p[d];
    for (uint32_t d = 0; d <= kPostMaxRadius; d++) k[d] = d <= radius ? (int32_t)(0.5 + p[d] / ww * 4194304.0) : 0;
}

// a post view's work for dec_view_post_kernel: src is the view's un-mirrored uint8 window in the decode scratch -- `planes` tight
// planes of w x h bytes, written by dec_resize_color_kernel<-1, *, false> -- and the rest the caller's destination as the records
// of the resize kernels describe it (planar: pixel_elems and hwc_flags 0; channels-last: plane_pitch 0)
struct DecViewPost {
    const uint8_t *src;
    uint8_t *dst;
    int64_t plane_pitch;
    int32_t pitch;
    uint32_t w, h, planes;
    uint32_t mirror;                 // FPNG_AMD_RESIZE_MIRROR of the view
    uint32_t pixel_elems, hwc_flags; // DecResizeHwc's
    uint32_t flags, radius, threshold, bits;
    int32_t k[kPostMaxRadius + 1];
    DecWarp warp; // the _views_warp calls' (view_warp.h); flags 0: none.  With a warp the gather mirrors and the store does not
    // the _views_tone calls' (view_tone.h); tone_op 0: none.  tone: the view's kToneBytes of the decode scratch -- uint32 h[4][256],
    // which dec_view_tone_hist_kernel counts, then the uint8 lut[3][256] that dec_view_tone_lut_kernel makes of them
    uint32_t *tone;
    uint32_t tone_op;
    float tone_factor;
    // the _views_enhance calls' (view_enhance.h); enhance_op 0: none
    uint32_t enhance_op;
    float enhance_factor;
};
static_assert(sizeof(DecViewPost) == 264 && offsetof(DecViewPost, enhance_op) == 256 && offsetof(DecViewPost, enhance_factor) == 260 && offsetof(DecViewPost, pitch) == 24 && offsetof(DecViewPost, k) == 68 && offsetof(DecViewPost, warp) == 136 &&
                  offsetof(DecViewPost, tone) == 240 && offsetof(DecViewPost, tone_factor) == 252,
              "DecViewPost layout");

// An exact grid as launch_dec_resize_color's, a workgroup per (record, tile of kResizeTileW x kResizeTileH): pre / h_pre count TILES.
// hwc: channels-last destinations.  mode 1: some record of the call has a warp (the instantiations that gather; 0: the post call's
// own); mode 2: some record has a tone op (the instantiations that gather and apply a table); mode 3: some record has an enhance op
// (those that also blend against a degenerate image).  false: a record without or with too many tiles; nothing is launched.
bool launch_dec_view_post(hipStream_t s, const DecViewPost *recs, const uint64_t *pre, const uint64_t *h_pre, uint32_t n, const DecFloat *flt, bool hwc, int mode = 0);

// The tone views of a call, in the order of their post records: refs[t].rec is tone view t's record of `recs`, refs[t].pre the chunks
// of kToneChunk samples of the tone views in front of it; refs[n].pre closes the sums.
struct DecToneRef {
    uint64_t pre;
    uint32_t rec, pad_;
};
static_assert(sizeof(DecToneRef) == 16, "DecToneRef layout");
FPNG_GRID_FN uint64_t exact_grid_pre(const DecToneRef &e) { return e.pre; } // (exact_grid.h: the refs are their own pre[])
// what one workgroup of dec_view_tone_hist_kernel counts: eight 64 x 16 tiles' worth of samples in all three planes -- 24576 (contrast:
// 8192) LDS atomics against the at most 768 (256) global ones of its flush; a 224 x 224 view is seven workgroups
constexpr uint32_t kToneChunk = 8 * kResizeTileW * kResizeTileH;
inline uint64_t tone_chunks(uint32_t w, uint32_t h) { return ((uint64_t)w * h + kToneChunk - 1) / kToneChunk; }
// refs .. refs + n (device; h_refs: the host's copy, n + 1 entries): the histograms -- zeroed on the stream by the caller -- and then
// the tables of those tone views.  false: a view without or with too many chunks; nothing is launched.
bool launch_dec_view_tone(hipStream_t s, const DecViewPost *recs, const DecToneRef *refs, const DecToneRef *h_refs, uint32_t n);

} // namespace fpng_amd
