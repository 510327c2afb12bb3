// resize_color.h -- the second stage of fpng_amd_decode_batch(_device)_planar_views_color and _hwc_views_color (include/fpng_amd.h):
// the views call's resize with a per-view 3 x 4 colour matrix between the resize's bytes and the element that is stored.  The rule
// of the resize is resize.h's, untouched; the rule of the colour step is color_apply() below -- the ONE text, run by
// dec_resize_color_kernel (resize_color.hip) for every pixel and by the host function fpng_amd_color_apply (decode_api.cpp) that
// the CPU tests judge against an exact restatement.
//
// r, g, b: the three bytes of a sample of the view, as floats (exact).  IEEE binary32, one fused multiply-add where written:
//
//   t_c = fmaf(m[c][2], b, fmaf(m[c][1], g, fmaf(m[c][0], r, m[c][3])))          c = 0, 1, 2: the FILE's channel
//   u_c = fminf(fmaxf(t_c, 0.0f), 255.0f)                                         (a t_c of -0.0f gives +0.0f)
//
// With finite entries of magnitude <= 65536 (the host refuses anything else) |t_c| < 2^26: never infinite, never NaN.
#pragma once
#include "decode.h"
#include "resize.h"
#include "resize_hwc.h"

#include <cmath>

namespace fpng_amd {

constexpr float kColorMaxEntry = 65536.0f; // |m[c][k]| <= this

// t_c of the rule for row (m0, m1, m2, m3) of a matrix, alone (yuv.h rounds it with quantize.h's clamp and rint)
FPNG_RESIZE_FN float color_mix(float m0, float m1, float m2, float m3, float r, float g, float b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_fmaf(m2, b, __builtin_fmaf(m1, g, __builtin_fmaf(m0, r, m3)));
#else
    return std::fmaf(m2, b, std::fmaf(m1, g, std::fmaf(m0, r, m3)));
#endif
}
// u_c of the rule for row (m0, m1, m2, m3) of a view's matrix.  (The clamp as two selects: which zero fmaxf returns for a t_c of
// -0.0f is left open by C; this returns +0.0f, on the host and on the device.)
FPNG_RESIZE_FN float color_apply(float m0, float m1, float m2, float m3, float r, float g, float b)
{
    const float t = color_mix(m0, m1, m2, m3, r, g, b);
    const float lo = t > 0.0f ? t : 0.0f;
    return lo < 255.0f ? lo : 255.0f;
}

// a view's work for dec_resize_color_kernel: the record of dec_resize_hwc_kernel -- for planar destinations r.dst / r.pitch /
// r.plane_pitch are the planar record's and pixel_elems / hwc_flags are 0 -- and the view's matrix
struct DecResizeColor {
    DecResizeHwc d;
    float m[3][4];
};
static_assert(sizeof(DecResizeColor) == 168 && offsetof(DecResizeColor, d) == 0 && offsetof(DecResizeColor, m) == 120, "DecResizeColor layout");

// An exact grid as launch_dec_resize_hwc's, a workgroup per (record, tile): pre / h_pre count TILES.  hwc: channels-last
// destinations (lds_bytes: the most resize_hwc_tile_lds() of the launch's records), else planar ones (the most resize_tile_lds()).
// false: a record without or with too many tiles, or lds_bytes out of range; nothing is launched.  any_alpha: some record of
// the launch carries an alpha op (view_alpha.h): the kernel's alpha instantiation.
bool launch_dec_resize_color(hipStream_t s, const DecResizeColor *recs, const uint64_t *pre, const uint64_t *h_pre, uint32_t n, uint32_t lds_bytes, const DecFloat *flt, uint32_t filters,
                             bool hwc, bool any_alpha = false);

} // namespace fpng_amd
